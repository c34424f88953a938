"""TEST INFRASTRUCTURE: rsk_conv_create_batch / rsk_conv_create_host (include/rsk_codec.h) restated with numpy
and a dict on top of tests/conv_ref.py, the scenarios the CPU and GPU tests share (side "cpu" = the host twin,
a device = the kernels), and the driver that runs either side with every output pre-filled with a sentinel.

The reference makes the SConn inside the packet walk (SubGroup::OnRecv -> newConn, server/SubGroup.cpp:31-68),
so the later packets of a batch find it; a new conv's DataStat starts at zero and alive
(conn/IConn.h:80-84)."""
from __future__ import annotations

import ctypes
import itertools

import numpy as np
import torch

from rsock_amd import _abi as A
from tests import conv_ref as R

NONE, SENT = R.NONE, R.SENT
SENT32 = int.from_bytes(bytes([SENT] * 4), "little")
VALID, DROP = A.RECV_VALID, A.RECV_DROP
COUNTER_COLS = ("cur_in", "cur_out", "prev_in", "prev_out", "alive")
TABLE_COLS = ("state", "conv", "dst", "id") + COUNTER_COLS
OPTIONAL = ("n_unknown", "new_rows", "new_first", "n_new", "n_full")
SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 4097, 70000)
CAPACITIES = R.CAPACITIES
FLAG_POINTS = ((65, 2), (4097, 257), (2049, 65536))  # (n, capacity) run under every flag combination


# ---- the restatement (semantics 1-8 of the header) -------------------------------------------------------
def unknown_batch(c, unknown):
    """The batch as the create sees it: a packet is looked at iff unknown == VALID, by its conv (dst, id)."""
    return {"status": np.asarray(unknown), "cmd": None, "hit": None, "conv": c["conv"], "dst": c.get("dst"),
            "id": c.get("id"), "ctl_kind": None, "ctl_arg": None}


def create_ref(cols, by_dst, by_id, c, conv_row, unknown, u_max, absent=()):
    """-> dict(cols = the table columns afterwards, conv_row, unknown, n_unknown, new_rows, new_first, n_new,
    n_full).  `absent`: counter columns the table does not have (left alone)."""
    cols = {k: (None if v is None else v.copy()) for k, v in cols.items()}
    conv_row, unknown = np.array(conv_row, np.uint32), np.array(unknown, np.int8)
    n = len(unknown)
    cu = unknown_batch(c, unknown)
    considered = np.full(n, DROP, np.int8)
    considered[np.nonzero(unknown == VALID)[0][:u_max]] = VALID
    first = R.first_arrivals(cu, considered, by_dst, by_id)
    vacant = np.nonzero((cols["state"] & A.CONN_LIVE) == 0)[0]
    n_new = min(len(first), len(vacant))
    rows, first_new = vacant[:n_new], first[:n_new]
    cols["state"][rows] = A.CONN_LIVE
    cols["conv"][rows] = c["conv"][first_new]
    if by_dst:
        cols["dst"][rows] = c["dst"][first_new]
    if by_id:
        cols["id"].reshape(-1, 8)[rows] = np.asarray(c["id"]).reshape(n, 8)[first_new]
    for k in COUNTER_COLS:
        if k not in absent:
            cols[k][rows] = 1 if k == "alive" else 0
    tmap, _ = R.table_map(cols, by_dst, by_id)
    _ex, _rst, keys = R.packet_keys(cu, by_dst, by_id)
    add = np.zeros(len(cols["state"]), np.uint32)
    for i in np.nonzero(unknown == VALID)[0].tolist():
        r = tmap.get(keys[i])
        if r is not None:
            conv_row[i], unknown[i] = r, DROP
            add[r] += 1
    if "cur_in" not in absent:
        cols["cur_in"] = cols["cur_in"] + add
    return {"cols": cols, "conv_row": conv_row, "unknown": unknown, "n_unknown": int((unknown == VALID).sum()),
            "new_rows": rows.astype(np.uint32), "new_first": first_new.astype(np.uint32), "n_new": n_new,
            "n_full": len(first) - n_new}


# ---- the driver ----------------------------------------------------------------------------------------
def make_table(rc, cols, device, by_dst, by_id, codec=None, absent=()):
    tab = R.make_table(rc, cols, device, by_dst, by_id, codec)
    for k in absent:
        setattr(tab, k, None)
    return tab


def table_columns(tab):
    return {k: tab.column(k) for k in TABLE_COLS if getattr(tab, k) is not None}


class Batch:
    """The device (or host) copies of a batch's key columns and of the resolve's in/out columns, with `slack`
    sentinel entries behind conv_row / unknown."""

    def __init__(self, c, conv_row, unknown, device, slack=3):
        self.n, self.device = len(unknown), device
        self.conv, self.dst, self.id = (R.tensor(c.get(k), device) for k in ("conv", "dst", "id"))
        self.conv_row, self.unknown = R.filled(self.n + slack, torch.int32, device), R.filled(self.n + slack, torch.int8, device)
        self.conv_row[:self.n] = R.tensor(np.asarray(conv_row, np.uint32), device)
        self.unknown[:self.n] = R.tensor(np.asarray(unknown, np.int8), device)


def run_create(rc, tab, b, u_max, codec=None, want=OPTIONAL, work=None, stream=None, slack=3):
    """One create on b's side with the optional outputs named in `want` pre-filled with SENT and `slack` spare
    entries behind the lists: -> dict of numpy outputs and "tail_ok"."""
    m = min(u_max, tab.capacity)
    dev = b.device
    o = {"n_unknown": R.filled(1, torch.int32, dev), "new_rows": R.filled(m + slack, torch.int32, dev),
         "new_first": R.filled(m + slack, torch.int32, dev), "n_new": R.filled(1, torch.int32, dev),
         "n_full": R.filled(1, torch.int32, dev)}
    o = {k: (v if k in want else None) for k, v in o.items()}
    work = tab.create_work(u_max) if work is None else work
    args = (tab, b.conv, b.conv_row[:b.n], b.unknown[:b.n], u_max, work)
    if codec is None:
        rc.conv_create_host(*args, id=b.id, dst=b.dst, **o)
    else:
        codec.conv_create_batch(*args, id=b.id, dst=b.dst, stream=stream, **o)
        torch.cuda.synchronize()
    return read_outputs(b, o)


def read_outputs(b, o):
    got = {"conv_row": R.host(b.conv_row, np.uint32)[:b.n], "unknown": R.host(b.unknown, np.int8)[:b.n]}
    ok = bool((R.host(b.conv_row, np.uint32)[b.n:] == SENT32).all()) and bool((R.host(b.unknown, np.uint8)[b.n:] == SENT).all())
    for k in ("n_unknown", "n_new", "n_full"):
        if o[k] is not None:
            got[k] = int(R.host(o[k], np.uint32)[0])
    for k in ("new_rows", "new_first"):
        if o[k] is not None:
            got[k + "_all"] = R.host(o[k], np.uint32)
    got["tail_ok"] = ok
    return got


def compare(got, want):
    assert got["tail_ok"]
    assert np.array_equal(got["conv_row"], want["conv_row"]), "conv_row"
    assert np.array_equal(got["unknown"], want["unknown"]), "unknown"
    for k in ("n_unknown", "n_new", "n_full"):
        if k in got:
            assert got[k] == want[k], (k, got[k], want[k])
    for k in ("new_rows", "new_first"):
        if k + "_all" in got:
            a = got[k + "_all"]
            assert np.array_equal(a[:want["n_new"]], want[k]), k
            assert bool((a[want["n_new"]:] == SENT32).all()), k + ": written past n_new"


def compare_table(tab, want_cols):
    for k in TABLE_COLS:
        if getattr(tab, k) is not None:
            assert np.array_equal(tab.column(k), want_cols[k]), k


def check_lookups(rc, tab, cols, by_dst, by_id, device, codec=None):
    """Every LIVE row's key, looked up through the resolve, finds the key's lowest row, and the index keeps
    rsk_conn.h's contract (the in-place inserts leave what a build leaves): on the index as it stands, and on a
    rebuilt copy of the table (the table itself goes on with the index as the create left it)."""
    live = np.nonzero(cols["state"] & A.CONN_LIVE)[0]
    tmap, _ = R.table_map(cols, by_dst, by_id)
    c = {"status": np.ones(len(live), np.int8), "cmd": None, "hit": None, "conv": cols["conv"][live],
         "dst": cols["dst"][live] if by_dst else None, "id": cols["id"].reshape(-1, 8)[live].ravel() if by_id else None,
         "ctl_kind": None, "ctl_arg": None}
    idw = R.id_words(cols["id"] if by_id else None, len(cols["state"]))
    want = np.array([tmap[R.row_key(cols, r, by_dst, by_id, idw)] for r in live.tolist()], np.uint32)
    rebuilt = tab.to(device)
    rebuilt.rebuild(codec)
    for t, what in ((tab, "index as the create left it"), (rebuilt, "index rebuilt")):
        R.check_index(t, cols, by_dst, by_id, what=what)
        if len(live) == 0:
            continue
        saved = None if t.cur_in is None else t.cur_in.clone()
        got = R.run_resolve(rc, t, c, device, codec, want=("n_unknown",), msg_mode="none")
        if saved is not None:
            t.cur_in.copy_(saved)
        assert np.array_equal(got["conv_row"], want) and got["n_unknown"] == 0, what


def resolve_create(rc, cols, c, by_dst, by_id, device, codec=None, u_max=None, absent=(), want=OPTIONAL, repeat=False):
    """Table from `cols`, one resolve of `c` (checked against conv_ref), then the create (called again as the
    header says when `repeat`), everything against create_ref with u_max >= n: every output, every table
    column bytewise, and the lookups of every table key.  -> (got, want, tab, batch)."""
    n = len(c["status"])
    tab = make_table(rc, cols, device, by_dst, by_id, codec, absent=absent)
    res_want = R.resolve_ref(cols, by_dst, by_id, c)
    res = R.run_resolve(rc, tab, c, device, codec, msg_mode="none")
    R.compare(res, res_want)
    after = dict(cols)
    if "cur_in" not in absent:
        after["cur_in"] = cols["cur_in"] + res_want["add"]
    u_max = max(n, 1) if u_max is None else u_max
    ref = create_ref(after, by_dst, by_id, c, res["conv_row"], res["unknown"], max(n, 1) if repeat else u_max, absent)
    b = Batch(c, res["conv_row"], res["unknown"], device)
    if not repeat:
        got = run_create(rc, tab, b, u_max, codec, want=want)
        compare(got, ref)
    else:
        rows, firsts, calls = [], [], 0
        work = tab.create_work(u_max)
        while True:
            got = run_create(rc, tab, b, u_max, codec, work=work)
            rows.append(got["new_rows_all"][:got["n_new"]])
            firsts.append(got["new_first_all"][:got["n_new"]])
            assert got["n_new"] <= u_max and bool((got["new_rows_all"][got["n_new"]:] == SENT32).all())
            calls += 1
            assert calls <= n + 1
            if not (got["n_unknown"] > 0 and got["n_full"] == 0):
                break
        got["calls"] = calls
        assert got["tail_ok"] and got["n_unknown"] == ref["n_unknown"]
        assert np.array_equal(np.concatenate(rows), ref["new_rows"]) and np.array_equal(np.concatenate(firsts), ref["new_first"])
        assert np.array_equal(got["conv_row"], ref["conv_row"]) and np.array_equal(got["unknown"], ref["unknown"])
    compare_table(tab, ref["cols"])
    check_lookups(rc, tab, ref["cols"], by_dst, by_id, device, codec)
    return got, ref, tab, b


# ---- shared scenarios ------------------------------------------------------------------------------------
def golden_server(name):
    g = R.golden_case(name)
    c = {"status": g["status"], "cmd": g["cmd"], "conv": g["conv"], "id": g["id"], "dst": g["dst"], "hit": None,
         "ctl_kind": None, "ctl_arg": None}
    leaves = len(np.unique(g["leaf"][g["leaf"] >= 0]))
    cols = R.random_columns(np.random.default_rng(1), max(1, leaves + 5))
    return g, c, cols, leaves


def scenario_golden_server(rc, name, device, codec=None):
    """One resolve -> create on an empty table of leaves + 5 rows gives the reference's recorded SConn per
    packet; conv_ref.scenario_golden_server needs two phases and a host step for the same."""
    g, c, cols, k = golden_server(name)
    got, ref, tab, _b = resolve_create(rc, cols, c, True, True, device, codec)
    data = (g["status"] == VALID) & (g["cmd"] == A.CMD_DATA)
    assert np.array_equal(got["conv_row"].view(np.int32), g["leaf"])
    assert got["n_unknown"] == 0 and got["n_full"] == 0 and got["n_new"] == k
    assert np.array_equal(got["new_first_all"][:k], R.first_arrivals(c, np.where(data, VALID, DROP)))
    assert np.array_equal(got["new_rows_all"][:k], np.arange(k))
    assert np.array_equal(tab.column("cur_in")[:k], np.bincount(g["leaf"][g["leaf"] >= 0], minlength=k).astype(np.uint32))
    return tab, c, g


def scenario_survives(rc, name, device, codec=None):
    """With no rebuild in between, a second resolve of the same columns finds every key; a rebuild followed by a
    resolve gives the same again."""
    tab, c, g = scenario_golden_server(rc, name, device, codec)
    for rebuilt in (False, True):
        if rebuilt:
            tab.rebuild(codec)
        got = R.run_resolve(rc, tab, c, device, codec, msg_mode="none")
        assert got["n_unknown"] == 0 and np.array_equal(got["conv_row"].view(np.int32), g["leaf"]), rebuilt


def scenario_random(rc, n, capacity, by_dst, by_id, device, codec=None, **kw):
    rng = np.random.default_rng(1000 * n + capacity + 7 * by_dst + 13 * by_id)
    cols, c = R.random_case(rng, n, capacity, by_dst, by_id, known=0.5, live=0.6, pool=min(capacity, 300))
    return resolve_create(rc, cols, c, by_dst, by_id, device, codec, **kw)


def new_keys_case(rng, n, keys, capacity, live_rows, by_dst=True, by_id=True):
    """A table with `live_rows` LIVE rows (keys of their own) and n DATA packets over `keys` distinct keys that
    the table does not hold, every key named by at least one packet when n >= keys."""
    cols = R.random_columns(rng, capacity, by_dst, by_id)
    cols["conv"][:] = np.arange(capacity, dtype=np.uint32) * np.uint32(2) + np.uint32(1)  # odd: no packet has one
    cols["state"][rng.permutation(capacity)[:live_rows]] = A.CONN_LIVE
    # groups of variants of one base key: the base, and one bit off in conv, in dst, in the IdBuf
    nvar = 2 + by_dst + by_id
    j = np.arange(keys)
    g, var = j // nvar, j % nvar
    kconv = ((g << 6) ^ np.where(var == 1, 2, 0)).astype(np.uint32)  # even: no row of the table has one
    kdst = np.full(keys, 0x0A000001, np.uint32)
    kid = np.tile(np.arange(1, 9, dtype=np.uint8), (keys, 1))
    if by_dst:
        kdst[var == 2] ^= np.uint32(0x00010000)
    if by_id:
        kid[var == 2 + by_dst, 5] ^= 0x40
    pick = rng.integers(0, keys, n)
    pick[rng.permutation(n)[:min(n, keys)]] = np.arange(min(n, keys))
    c = {"status": np.ones(n, np.int8), "cmd": None, "hit": None, "conv": kconv[pick], "dst": kdst[pick] if by_dst else None,
         "id": kid[pick].ravel() if by_id else None, "ctl_kind": None, "ctl_arg": None}
    return cols, c


def scenario_full(rc, kind, device, codec=None):
    rng = np.random.default_rng(61)
    if kind == "fewer":
        cols, c = new_keys_case(rng, 3000, 200, 300, 260)  # 40 vacant rows for 200 keys
    elif kind == "none":
        cols, c = new_keys_case(rng, 3000, 50, 300, 300)
    elif kind == "cap1_vacant":
        cols, c = new_keys_case(rng, 500, 7, 1, 0)
    else:  # cap1_live
        cols, c = new_keys_case(rng, 500, 7, 1, 1)
    got, ref, _tab, _b = resolve_create(rc, cols, c, True, True, device, codec)
    keys = len(R.first_arrivals(c, c["status"]))
    vacant = int(((cols["state"] & A.CONN_LIVE) == 0).sum())
    assert got["n_new"] == min(keys, vacant) and got["n_full"] == keys - got["n_new"] > 0
    left = got["unknown"] == VALID
    assert got["n_unknown"] == int(left.sum()) > 0 and bool((got["conv_row"][left] == NONE).all())
    assert bool((got["conv_row"][~left] != NONE).all())


def scenario_u_max(rc, u_max, device, codec=None):
    rng = np.random.default_rng(67 + u_max)
    n, keys = (700, 60) if u_max == 1 else (5000, 300)
    cols, c = new_keys_case(rng, n, keys, 400, 37)
    c["status"][rng.random(n) < 0.1] = DROP
    got, _ref, _tab, _b = resolve_create(rc, cols, c, True, True, device, codec, u_max=u_max, repeat=True)
    assert got["calls"] > 1 and got["n_unknown"] == 0


def scenario_u_max_full(rc, device, codec=None):
    """The sequence of calls ends on n_full > 0 with what one big call on the same vacant rows gives, as long as
    the vacant rows run out inside one call's keys: here every call but the last creates all of its keys."""
    rng = np.random.default_rng(71)
    cols, c = new_keys_case(rng, 64 * 4, 64 * 4, 300, 300 - 64 * 3)
    got, _ref, _tab, _b = resolve_create(rc, cols, c, True, True, device, codec, u_max=64, repeat=True)
    assert got["n_full"] > 0 and got["n_unknown"] > 0


def scenario_skew(rc, kind, device, codec=None):
    rng = np.random.default_rng(73)
    n = 4097
    for by_dst, by_id in R.FLAG_COMBOS:
        cols, c = new_keys_case(rng, n, 1 if kind == "one_key" else n, 5000, 500, by_dst, by_id)
        got, _ref, tab, _b = resolve_create(rc, cols, c, by_dst, by_id, device, codec)
        k = 1 if kind == "one_key" else n
        assert got["n_new"] == k and got["n_unknown"] == 0
        cur = tab.column("cur_in")[got["new_rows_all"][:k].astype(np.int64)]
        assert cur.tolist() == ([n] if kind == "one_key" else [1] * n)


def scenario_reads(rc, device, codec=None):
    """Key fields of packets that are not unknown are poisoned after the resolve and change nothing; a CONV_RST
    packet naming a conv born in the call keeps NONE."""
    rng = np.random.default_rng(79)
    n, cap = 5000, 600
    cols, c = R.random_case(rng, n, cap, True, True, known=0.5, live=0.5, pool=200)
    # CONV_RST packets whose body names the key of a DATA packet that is unknown (a conv about to be born)
    tab = make_table(rc, cols, device, True, True, codec)
    res = R.run_resolve(rc, tab, c, device, codec, msg_mode="none")
    unk = np.nonzero(res["unknown"] == VALID)[0]
    rst = np.nonzero((c["ctl_kind"] == A.CTL_CONV_RST) & ~R.examined(c))[0]
    assert len(unk) > 200 and len(rst) > 100
    src = rng.choice(unk, len(rst))
    c["ctl_arg"][rst] = c["conv"][src].astype(np.uint64)
    c["dst"][rst] = c["dst"][src]
    c["id"].reshape(-1, 8)[rst] = c["id"].reshape(-1, 8)[src]
    want = R.resolve_ref(cols, True, True, c)
    after = dict(cols, cur_in=cols["cur_in"] + want["add"])
    ref = create_ref(after, True, True, c, want["conv_row"], want["unknown"], n)
    assert ref["n_new"] > 50 and bool((ref["conv_row"][rst] == NONE).all())
    skip = want["unknown"] != VALID
    outs = []
    for poison in (None, 0x00, 0xFF, 0x5A):
        p = {k: (None if v is None else v.copy()) for k, v in c.items()}
        tab = make_table(rc, cols, device, True, True, codec)
        res = R.run_resolve(rc, tab, p, device, codec, msg_mode="none")
        R.compare(res, want)
        if poison is not None:
            p["conv"][skip] = int.from_bytes(bytes([poison] * 4), "little")
            p["dst"][skip] = int.from_bytes(bytes([poison] * 4), "little")
            p["id"].reshape(-1, 8)[skip] = poison
        b = Batch(p, res["conv_row"], res["unknown"], device)
        got = run_create(rc, tab, b, n, codec)
        compare(got, ref)
        compare_table(tab, ref["cols"])
        outs.append(got)
    assert bool((outs[0]["conv_row"][rst] == NONE).all())


def scenario_optional_outputs(rc, device, codec=None):
    rng = np.random.default_rng(83)
    cols, c = R.random_case(rng, 1500, 200, True, True, known=0.5, live=0.5, pool=80)
    for k in range(len(OPTIONAL) + 1):
        for want in itertools.combinations(OPTIONAL, k):
            resolve_create(rc, cols, c, True, True, device, codec, want=want)
    resolve_create(rc, cols, c, True, True, device, codec, absent=("cur_in",))
    resolve_create(rc, cols, c, True, True, device, codec, absent=COUNTER_COLS)
    resolve_create(rc, cols, c, True, True, device, codec, absent=COUNTER_COLS, want=())
    # n == 0: the given counts are written, nothing else
    tab = make_table(rc, cols, device, True, True, codec)
    before = table_columns(tab)
    index = tab.index.clone()
    b = Batch({"conv": np.zeros(0, np.uint32), "dst": np.zeros(0, np.uint32), "id": np.zeros(0, np.uint8)}, [], [], device)
    for want in (OPTIONAL, ("n_new",), ()):
        got = run_create(rc, tab, b, 5, codec, want=want)
        assert got["tail_ok"] and all(got[k] == 0 for k in ("n_unknown", "n_new", "n_full") if k in want)
        for k in ("new_rows", "new_first"):
            assert k not in want or bool((got[k + "_all"] == SENT32).all())
    compare_table(tab, before)
    assert bool((tab.index == index).all())
    L = rc.lib()
    o = A.ConvCreateOut()
    i = A.ConvCreateIn(None, None, None, 1, tab.create_work(1).data_ptr())
    ctx = () if codec is None else (codec._ctx,)
    fn = L.rsk_conv_create_host if codec is None else L.rsk_conv_create_batch
    assert fn(*ctx, ctypes.byref(tab.abi()), ctypes.byref(tab.abi_rows()), 0, ctypes.byref(i), ctypes.byref(o),
              1 if codec is None else None) == A.OK


def scenario_determinism(rc, device, codec=None):
    outs = []
    for _ in range(2):
        got, _ref, tab, _b = scenario_random(rc, 4097, 257, True, True, device, codec)
        outs.append((got, table_columns(tab)))
    (g0, t0), (g1, t1) = outs
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    for k in t0:
        assert t0[k].tobytes() == t1[k].tobytes(), k


def check_einval(rc, device, codec=None):
    """Every RSK_EINVAL of the create, with the outputs and the table untouched by a rejected call."""
    L = rc.lib()
    tabs, a, n = R.einval_fixture(rc, device, codec)
    server, client = tabs[(True, True)], tabs[(False, False)]
    ctx = () if codec is None else (codec._ctx,)
    tail = (1,) if codec is None else (None,)
    fn = L.rsk_conv_create_host if codec is None else L.rsk_conv_create_batch
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
    p = lambda k: a[k].data_ptr()  # noqa: E731
    unk = R.tensor(np.full(n, DROP, np.int8), device)
    work = server.create_work(4)
    lists = R.filled(8, torch.int32, device)

    def cin(**kw):
        d = dict(id=p("id"), conv=p("conv"), dst=p("dst"), u_max=4, work=work.data_ptr())
        d.update(kw)
        return A.ConvCreateIn(*[d[f] for f, _ in A.ConvCreateIn._fields_])

    def cout(**kw):
        d = dict(conv_row=p("row"), unknown=unk.data_ptr(), n_unknown=p("cnt"), new_rows=lists.data_ptr(),
                 new_first=lists.data_ptr() + 16, n_new=None, n_full=None)
        d.update(kw)
        return A.ConvCreateOut(*[d[f] for f, _ in A.ConvCreateOut._fields_])

    E = A.EINVAL
    cases = [("null tab", None, server.abi_rows(), n, cin(), cout()), ("null rows", server.abi(), None, n, cin(), cout()),
             ("null in", server.abi(), server.abi_rows(), n, None, cout()),
             ("null out", server.abi(), server.abi_rows(), n, cin(), None),
             ("null work", server.abi(), server.abi_rows(), n, cin(work=None), cout()),
             ("null work, n 0", server.abi(), server.abi_rows(), 0, cin(work=None), cout()),
             ("u_max 0", server.abi(), server.abi_rows(), n, cin(u_max=0), cout()),
             ("u_max too large", server.abi(), server.abi_rows(), n, cin(u_max=(1 << 24) + 1), cout()),
             ("conv_row", server.abi(), server.abi_rows(), n, cin(), cout(conv_row=None)),
             ("unknown", server.abi(), server.abi_rows(), n, cin(), cout(unknown=None)),
             ("in.conv", server.abi(), server.abi_rows(), n, cin(conv=None), cout()),
             ("in.dst", server.abi(), server.abi_rows(), n, cin(dst=None), cout()),
             ("in.id", server.abi(), server.abi_rows(), n, cin(id=None), cout()),
             ("in.id misaligned", server.abi(), server.abi_rows(), n, cin(id=p("id") + 4), cout()),
             ("work misaligned", server.abi(), server.abi_rows(), n, cin(work=work.data_ptr() + 8), cout()),
             ("n too large", server.abi(), server.abi_rows(), A.MAX_BATCH + 1, cin(), cout())]
    for field, val in (("flags", 4), ("flags", 0x80000003), ("capacity", 0), ("capacity", A.CONN_MAX_ROWS + 1),
                       ("state", None), ("conv", None), ("index", None), ("dst", None), ("id", None)):
        t = server.abi()
        setattr(t, field, val)
        cases.append((f"tab.{field}={val}", t, server.abi_rows(), n, cin(), cout()))
    for field in ("state", "conv", "dst", "id"):
        r = server.abi_rows()
        setattr(r, field, getattr(client.abi(), "conv"))
        cases.append((f"rows.{field} not the table's", server.abi(), r, n, cin(), cout()))
        r = server.abi_rows()
        setattr(r, field, None)
        cases.append((f"rows.{field} NULL", server.abi(), r, n, cin(), cout()))
    t, r = server.abi(), server.abi_rows()
    t.id += 4
    r.id += 4
    cases.append(("tab.id misaligned", t, r, n, cin(), cout()))
    before = table_columns(server)

    def untouched():
        if codec is not None:
            torch.cuda.synchronize()
        return (all(bool((x.cpu().view(torch.uint8) == SENT).all()) for x in (a["row"], a["cnt"], lists))
                and bool((unk.cpu() == DROP).all()))

    for label, t, r, nn, i, o in cases:
        if codec is None and "id misaligned" in label:  # the host twin reads ids bytewise
            continue
        assert fn(*ctx, ref(t), ref(r), nn, ref(i), ref(o), *tail) == E, label
        assert untouched(), label
    if codec is not None:
        assert L.rsk_conv_create_batch(None, ref(server.abi()), ref(server.abi_rows()), n, ref(cin()), ref(cout()), None) == E
    compare_table(server, before)
    # the valid calls do run: a client's rows need no dst / id, and no packet is unknown
    cw = client.create_work(4)
    assert fn(*ctx, ref(client.abi()), ref(A.ConvRows(client.state.data_ptr(), client.conv.data_ptr(), None, None)), n,
              ref(cin(dst=None, id=None, work=cw.data_ptr())), ref(cout()), *tail) == A.OK
    assert fn(*ctx, ref(server.abi()), ref(server.abi_rows()), n, ref(cin()), ref(cout()), *tail) == A.OK
    if codec is not None:
        torch.cuda.synchronize()
    assert R.host(a["cnt"], np.uint32)[0] == 0 and bool((R.host(a["row"], np.uint8) == SENT).all())
    compare_table(server, before)
    assert L.rsk_conv_create_bytes(0, 4) == 0 and L.rsk_conv_create_bytes((1 << 24) + 1, 4) == 0
    assert L.rsk_conv_create_bytes(4, 0) == 0 and L.rsk_conv_create_bytes(4, A.CONN_MAX_ROWS + 1) == 0
    # the documented formula: 4 * (16 + M + P + u_max + 2 min(u_max, C)) rounded up to 16
    for u, cap in ((1, 1), (3, 2), (64, 1000), (65, 7), (70000, 65536), (1 << 24, 1 << 20)):
        pw = 4
        while pw < 2 * u:
            pw *= 2
        mw = (2 * ((u + 63) // 64) + 3) // 4 * 4
        assert L.rsk_conv_create_bytes(u, cap) == (4 * (16 + mw + pw + u + 2 * min(u, cap)) + 15) // 16 * 16, (u, cap)


# ---- exact counts of the create on rows that collide in the LDS aggregator -------------------------------------
def scenario_band_create(rc, n, pattern, device, codec=None, cache=None):
    """A 2^18-row client table whose only vacant rows are conv_ref.band_rows(): the convs born in the call take
    them in first-arrival order, so the packets' rows share one run of the count pass's LDS table.  conv_row,
    the lists and cur_in (a new conv starts at zero) against np.bincount, exactly."""
    tab, cols, band = R.band_table(rc, device, codec, cache, vacant_band=True)
    tab.load(**{k: cols[k] for k in TABLE_COLS if cols.get(k) is not None})
    tab.rebuild(codec)
    want_row = R.band_packets(band, n, pattern)
    # the key of a packet is the conv the band's row held (not LIVE: the table does not know it)
    c = {"conv": cols["conv"][want_row], "dst": None, "id": None}
    _u, first, inv = np.unique(want_row, return_index=True, return_inverse=True)
    rank = np.argsort(np.argsort(first))  # distinct key -> its place in first-arrival order
    row = band[rank[inv]]
    k = len(first)
    b = Batch(c, np.full(n, NONE, np.uint32), np.full(n, VALID, np.int8), device)
    got = run_create(rc, tab, b, n, codec)
    assert got["tail_ok"] and got["n_unknown"] == 0 and got["n_full"] == 0 and got["n_new"] == k
    assert np.array_equal(got["conv_row"], row) and bool((got["unknown"] == DROP).all())
    assert np.array_equal(got["new_rows_all"][:k], band[:k]) and np.array_equal(got["new_first_all"][:k], np.sort(first))
    state = cols["state"].copy()
    state[band[:k]] = A.CONN_LIVE
    cur = cols["cur_in"].copy()
    cur[band[:k]] = 0
    cur += np.bincount(row, minlength=len(cur)).astype(np.uint32)
    assert np.array_equal(tab.column("state"), state)
    assert np.array_equal(tab.column("cur_in"), cur), np.nonzero(tab.column("cur_in") != cur)[0][:8]
    assert np.array_equal(tab.column("conv")[band[:k]], c["conv"][np.sort(first)])
    return k
