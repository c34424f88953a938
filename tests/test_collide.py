"""CPU: tests/collide.py is what it says.  The restated hashes carry the constants of the sources (read out of
their text, so a change of a hash fails here and names the module to update), the constructors give keys with the
promised home, fingerprint or hash, the host twin's index holds a constructed cluster as one run from the
predicted entry, index_invariant refuses the indexes of broken inserts, and tests/demux_ref.segments_ref equals
the oracle on the demux tests' shapes."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import collide as X
from tests import conn_ref as R
from tests import demux_ref as D
from tests.test_demux_oracle import ALL, make_case

# every field selection of tests/test_gpu_demux.py's FIELDS (restated: a CPU module does not import a GPU one)
FIELDS = [ALL, A.DEMUX_CONN_KEY, A.DEMUX_ID | A.DEMUX_CONV | A.DEMUX_DST, A.DEMUX_CONV, 0, ALL | A.DEMUX_CMD_BARRIER,
          A.DEMUX_CONN_KEY | A.DEMUX_CMD_BARRIER, A.DEMUX_CMD_BARRIER, ALL | A.DEMUX_GROUP_BARRIER,
          A.DEMUX_ID | A.DEMUX_GROUP_BARRIER]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rsock_amd", "csrc")
STALE = "tests/collide.py restates this hash: update it together with "


def text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def body(src, head):
    """The text of the function whose definition starts with `head`, up to its closing brace at column 0."""
    at = src.index(head)
    return src[at: src.index("\n}", at)]


def hexes(s):
    return [int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]+)u?l*\b", s)]


# ---- the restatements carry the sources' constants ---------------------------------------------------------------
def test_conn_hash_constants():
    src = text("rsk_conn.h")
    mix = body(src, "RSK_CONN_HD uint64_t conn_mix")
    assert hexes(mix) == [X.MIX_M1, X.MIX_M2], STALE + "rsk_conn.h's conn_mix"
    assert tuple(int(s) for s in re.findall(r"x \^= x >> (\d+);", mix)) == X.MIX_SHIFTS, STALE + "rsk_conn.h's conn_mix"
    home = body(src, "RSK_CONN_HD uint32_t conn_home")
    assert hexes(home) == [X.GOLDEN] and re.search(r">> 32\) & \(slots - 1u\)", home), STALE + "rsk_conn.h's conn_home"
    slots = body(src, "RSK_CONN_HD uint32_t conn_slots")
    assert re.search(r"s = 4u;\s*while \(s < 2u \* capacity\) s <<= 1;", slots), STALE + "rsk_conn.h's conn_slots"
    assert hexes(re.search(r"kConnEmpty = (\w+);", src).group(1)) == [X.EMPTY]
    assert A.CONN_LIVE == X.LIVE and A.CONN_MAX_ROWS * 2 == X.WIDE


def test_offers_hash_and_side_tables():
    """What tuples_at, the dedup / offers / new-group tables' homes and pick_ref.group_taken rely on."""
    src = text("rsk_conn_create.h")
    why = STALE + "rsk_conn_create.h's tuple_key / tuple_ports"
    assert re.search(r"tuple_key\(uint32_t src, uint32_t dst\) \{ return \(\(uint64_t\)src << 32\) \| dst; \}", src), why
    assert re.search(r"tuple_ports\(uint16_t sp, uint16_t dp\) \{ return \(\(uint64_t\)sp << 16\) \| dp; \}", src), why
    cs = body(text("rsk_conv_create.h"), "RSK_CONN_HD uint32_t create_slots")
    assert re.search(r"s = 4u;\s*while \(s < 2u \* u\) s <<= 1;", cs), STALE + "rsk_conv_create.h's create_slots"
    for unit, probes in (("rsk_conn_create.hip", ("conn_home(key, id, ds)", "conn_home(tk, tp, ds)", "conn_home(0ull, id, ds)",
                                                  "conn_home(0ull, id, a.slots)")),
                         ("rsk_conv_create.hip", ("conn_home(key, id, dslots)",)), ("rsk_pick.hip", ("conn_home(0ull, id, a.slots)",)),
                         ("rsk_host.cpp", ("conn_home(0ull, id, slots)", "conn_home(key, id, dslots)"))):
        t = text(unit)
        assert all(p in t for p in probes), STALE + unit + "'s probes (every side table starts at rsk_conn.h's conn_home)"
    lay = body(text("rsk_pick.h"), "RSK_CONN_HD PickLayout pick_layout")
    for line in ("l.cand = kPickHdr;", "l.pos = l.cand + c4;", "l.lead = l.pos + c4;", "l.group = l.lead + (by_id ? slots : 0u);",
                 "l.words = l.group + (by_id ? 4u * slots : 0u);"):
        assert line in lay, "tests/pick_ref.group_taken restates rsk_pick.h's pick_layout: update it together with it"
    assert re.search(r"constexpr uint32_t kPickHdr = 4u;", text("rsk_pick.h"))


def test_demux_hash_constants():
    src = text("rsk_demux.hip")
    kh = body(src, "__device__ __forceinline__ uint64_t key_hash")
    why = STALE + "rsk_demux.hip's key_hash"
    assert hexes(kh) == [X.DM_C1, X.DM_C2, X.DM_C3, X.DM_C4, X.DM_FIN_MUL], why
    assert tuple(int(s) for s in re.findall(r"h \^= h >> (\d+);", kh)) == X.DM_FIN_SHIFTS, why
    fields = re.search(r"\(\(uint64_t\)k\.ep \| \(uint64_t\)k\.xf << 32\) \* \w+ \^ k\.id \* \w+ \^\s*k\.ck \* \w+ \^ "
                       r"\(\(uint64_t\)k\.conv \| \(uint64_t\)k\.dst << 32\) \* \w+;", kh)
    assert fields, why
    assert re.search(r"uint32_t h = \(uint32_t\)\(hv \^ \(hv >> (\d+)\)\) & \(kLtab - 1u\);", src).group(1) == str(X.DM_LDS_SHIFT), why
    assert len(re.findall(r"uint32_t h = \(uint32_t\)hv & mask", src)) == 2, why  # global_probe and k_dm_gep
    assert len(re.findall(r"fp = \(uint32_t\)\(hv >> 32\)", src)) == 3, why
    k_block = int(re.search(r"constexpr int kBlock = (\d+);", src).group(1))
    items = int(re.search(r"constexpr uint32_t kInsItems = (\d+);", src).group(1))
    assert re.search(r"kInsTile = kBlock \* kInsItems;", src) and re.search(r"kLtab = 2 \* kInsTile;", src), why
    assert k_block * items == X.DM_INS_TILE and 2 * k_block * items == X.DM_LDS_SLOTS, why
    ts = body(src, "uint32_t table_size(uint32_t n)")
    assert re.search(r"t = 64;\s*while \(t < 2ull \* n\) t <<= 1;", ts), STALE + "rsk_demux.hip's table_size"


def test_aggregator_constants():
    src = text("rsk_tile_dev.h")
    why = STALE + "rsk_tile_dev.h's tile_count_rows"
    m = re.search(r"uint32_t s = \(row\[k\] \* (\w+)\) >> \(32u - \(unsigned\)__builtin_ctz\(kSlots\)\);", src)
    assert m and hexes(m.group(1)) == [X.AGG_MUL], why
    assert re.search(r"kSlots = 2u \* PER \* kTileBlock;", src), why
    block = int(re.search(r"constexpr unsigned kTileBlock = (\d+);", src).group(1))
    for user in ("rsk_conv.hip", "rsk_conv_create.hip"):  # the callers' tiles: RowAgg<kPer>
        t = text(user)
        assert "RowAgg<kPer>" in t and re.search(r"constexpr unsigned kBlock = rsk::kTileBlock;", t), why
        assert 2 * int(re.search(r"constexpr unsigned kPer = (\d+);", t).group(1)) * block == X.AGG_SLOTS, why


# ---- the constructors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("home", [R.WRAP_HOME, R.INNER_HOME, 0, 1 << 20])
def test_index_constructors(home):
    k = 300
    want = lambda s: home % s  # noqa: E731
    for idw in (0, 0x0123456789ABCDEF):
        keys = X.keys_at(home, k, idw)
        assert len(set(keys.tolist())) == k
        for slots in (4, 128, 2048, 1 << 21):
            assert {X.conn_home(int(x), idw, slots) for x in keys} == {want(slots)}
    ids = X.ids_at(home, k)
    assert len(set(ids.tolist())) == k and {X.group_home(int(i), 1025) for i in ids} == {want(4096)}
    ids = X.ids_at(home, k, key=77)
    assert len(set(ids.tolist())) == k and {X.conn_home(77, int(i), 512) for i in ids} == {want(512)}
    src, dst, sp, dp = X.tuples_at(home, k)
    tk = (src.astype(np.uint64) << np.uint64(32)) | dst
    tp = (sp.astype(np.uint64) << np.uint64(16)) | dp
    assert len({(int(a), int(b)) for a, b in zip(tk, tp)}) == k
    assert {X.conn_home(int(a), int(b), 8192) for a, b in zip(tk, tp)} == {want(8192)}
    for slots, n in ((1024, 1025), (8192, 300)):
        convs = X.convs_at(home, n, slots)
        assert len(set(convs.tolist())) == n and {X.conn_home(int(c), 0, slots) for c in convs} == {want(slots)}
    assert all(X.unmix(X.conn_mix(x)) == x for x in (0, 1, X.M64, 0x10002711_9C40))


def test_demux_constructors():
    ids, ck = X.same_hash(600)
    assert len({(int(i), int(c)) for i, c in zip(ids, ck)}) == 600
    for ep, conv, dst in ((0, 0, 0), (7, 0, 0), (3, 9, 0x0A000001)):
        assert len({X.key_hash(ep, int(i), int(c), conv, dst) for i, c in zip(ids, ck)}) == 1
    mask = X.dm_table_slots(1500) - 1
    assert mask == 4095 and X.dm_table_slots(3) == 64 and X.dm_table_slots(2048) == 4096
    homes = [(mask - 1 + 5 * j) & mask for j in range(100)]
    keys = X.same_fp(100, homes, mask)
    hv = [X.key_hash(ck=int(c)) for c in keys]
    assert len(set(keys.tolist())) == 100 and {X.dm_fp(h) for h in hv} == {0xC0111DE5}
    assert [X.dm_home(h, mask) for h in hv] == homes
    keys = X.same_home(100, mask - 1, mask, ep=4)
    hv = [X.key_hash(ep=4, ck=int(c)) for c in keys]
    assert {X.dm_home(h, mask) for h in hv} == {mask - 1} and len({X.dm_fp(h) for h in hv}) == 100
    keys = X.epoch_keys(0xFEEDFACE_00000FFE, range(6))
    assert len(set(keys.tolist())) == 6
    assert {X.key_hash(ep=e, ck=int(c)) for e, c in enumerate(keys)} == {0xFEEDFACE_00000FFE}
    idw = X.ids_same_fp_home(300, mask)
    hv = [X.key_hash(idw=int(i)) for i in idw]
    assert len(set(idw.tolist())) == 300 and {X.dm_fp(h) for h in hv} == {0x1DB0F5ED}
    assert {X.dm_home(h, mask) for h in hv} == {mask - 1} and len({X.dm_lds_home(h) for h in hv}) == 1
    assert all(X.dm_unfin(X.dm_fin(x)) == x for x in (0, 1, X.M64, 0x10002711_9C40))


def test_aggregator_band():
    """More distinct rows than one 2048-packet tile holds, in one run of the LDS table that crosses its end."""
    cap = 1 << 18
    narrow, wide = X.rows_in_band(cap, X.AGG_SLOTS - 8, 16), X.rows_in_band(cap, X.AGG_SLOTS - 32, 40)
    assert len(narrow) == 1025 and len(wide) == 2560
    h = X.agg_home(wide)
    assert bool(((h >= X.AGG_SLOTS - 32) | (h < 8)).all()) and bool((h < 8).any()) and bool((h >= X.AGG_SLOTS - 32).any())
    assert int(X.agg_home(1)) == (X.AGG_MUL >> 20)


# ---- the host twin holds a constructed cluster as one run, and the contract's checker refuses broken indexes --------
@pytest.mark.parametrize("by_id", [False, True])
def test_host_twin_holds_the_cluster_as_one_run(by_id):
    cap = 257
    cols, home, distinct, _ = R.cluster_table(cap, "one_home", by_id, True)
    tab, ndup = R.built_table(rc, cols, by_id, "cpu")
    index = tab.index.numpy().view(np.uint32)
    slots = X.conn_slots(cap)
    assert ndup == 0 and distinct == cap and len(index) == slots == 1024
    assert set(np.nonzero(index != X.EMPTY)[0].tolist()) == {(slots - 3 + i) % slots for i in range(cap)}
    X.one_run(index, home, cap)
    assert R.check_index(tab, cols, by_id) == cap


def test_linear_insert_is_a_sequential_insert():
    """index_invariant's expected occupancy against the textbook loop, in two insertion orders."""
    rng = np.random.default_rng(1)
    for slots, k, spread in ((8, 4, 8), (64, 32, 5), (1024, 500, 40), (1024, 512, 1024), (16, 1, 16)):
        homes = (slots - 3 + rng.integers(0, spread, k)) % slots
        for order in (homes, homes[::-1]):
            taken = np.zeros(slots, bool)
            for h in order.tolist():
                while taken[h]:
                    h = (h + 1) % slots
                taken[h] = True
            assert np.array_equal(X.linear_insert(slots, homes), taken), (slots, k, spread)


def python_index(cols, by_id, probe_wraps=True, compare_keys=True):
    """A sequential index build in Python over the LIVE rows in row order; the two switches break it."""
    cap = len(cols["state"])
    slots = X.conn_slots(cap)
    idw = R.id_words(cols["id"] if by_id else None, cap)
    index = np.full(slots, X.EMPTY, np.uint32)
    for r in np.nonzero(cols["state"] & A.CONN_LIVE)[0].tolist():
        s = X.conn_home(int(cols["conn_key"][r]), int(idw[r]), slots)
        while True:
            e = int(index[s])
            if e == X.EMPTY:
                index[s] = r
                break
            if compare_keys and cols["conn_key"][e] == cols["conn_key"][r] and idw[e] == idw[r]:
                break
            s += 1
            if s == slots:
                if not probe_wraps:
                    break  # the row is lost
                s = 0
    return index


def python_lookup(index, cols, by_id, key, idw, max_steps=None):
    cap = len(cols["state"])
    slots = len(index)
    ids = R.id_words(cols["id"] if by_id else None, cap)
    s = X.conn_home(int(key), int(idw), slots)
    for _ in range(slots if max_steps is None else max_steps):
        e = int(index[s])
        if e >= cap:
            break
        if cols["conn_key"][e] == key and ids[e] == idw:
            return e
        s = (s + 1) & (slots - 1)
    return R.NONE


@pytest.mark.parametrize("by_id", [False, True])
def test_checkers_refuse_broken_tables(by_id):
    """The Python model passes the checks the scenarios make; the model with a probe that stops at the last entry,
    with an insert that takes the first free entry without comparing keys, and with a lookup capped at 64 steps
    each fail one of them."""
    cap = 65
    cols, home, distinct, (pk, pi) = R.cluster_table(cap, "duplicates", by_id, True)
    args = (cap, cols["state"], cols["conn_key"], R.id_words(cols["id"], cap) if by_id else None, by_id)
    good = python_index(cols, by_id)
    assert X.index_invariant(good, *args) == distinct
    X.one_run(good, home, distinct)
    tmap, _ = R.table_map(cols["state"], cols["conn_key"], cols["id"] if by_id else None)
    want = R.resolve_ref(tmap, np.ones(len(pk), np.int8), pk, id=pi.view(np.uint8) if by_id else None)[0]
    look = lambda index, **kw: np.array([python_lookup(index, cols, by_id, k, i, **kw) for k, i in zip(pk, pi)], np.uint32)  # noqa: E731
    assert np.array_equal(look(good), want)
    with pytest.raises(AssertionError):
        X.index_invariant(python_index(cols, by_id, probe_wraps=False), *args)
    with pytest.raises(AssertionError):
        X.index_invariant(python_index(cols, by_id, compare_keys=False), *args)
    cols, home, distinct, (pk, pi) = R.cluster_table(257, "one_home", by_id, True)  # a run longer than the cap
    good = python_index(cols, by_id)
    tmap, _ = R.table_map(cols["state"], cols["conn_key"], cols["id"] if by_id else None)
    want = R.resolve_ref(tmap, np.ones(len(pk), np.int8), pk, id=pi.view(np.uint8) if by_id else None)[0]
    assert np.array_equal(look(good), want) and not np.array_equal(look(good, max_steps=64), want)
    twin, _ = R.built_table(rc, cols, by_id, "cpu")
    assert np.array_equal(twin.index.numpy().view(np.uint32) != X.EMPTY, good != X.EMPTY)


# ---- the hash-free demux reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("fields", FIELDS)
@pytest.mark.parametrize("shape", [(0, 1, 0.0, 1.0), (1, 1, 0.0, 1.0), (500, 3, 0.05, 0.9), (3000, 40, 0.01, 0.7),
                                   (2000, 2000, 0.0, 1.0), (800, 5, 0.5, 1.0), (300, 4, 0.0, 0.0), (400, 7, 1.0, 1.0)])
def test_segments_ref_equals_oracle(oracle, fields, shape):
    n, nkeys, p_ctrl, p_valid = shape
    rng = np.random.default_rng(n * 31 + nkeys + fields)
    case = make_case(rng, n, nkeys, p_ctrl, p_valid)
    assert D.segments_ref(case[0], case[1], fields, *case[2:]) == oracle.demux_batch(case[0], case[1], fields, *case[2:])


# ---- the constructed keys are adversarial for the device-only tables: Python models of them, and their mutants ------
def demux_model(status, fields, idw, ckey, trust_fingerprint=False):
    """rsk_demux.hip's global table for a batch without barriers, one packet at a time: an entry is (fingerprint,
    first packet); a matching fingerprint is confirmed on the full key -- or trusted, the mutant."""
    n = len(status)
    mask = X.dm_table_slots(n) - 1
    table, segs = {}, {}
    for i in np.nonzero(status == A.RECV_VALID)[0].tolist():
        key = (int(idw[i]) if fields & A.DEMUX_ID else 0, int(ckey[i]) if fields & A.DEMUX_CONN_KEY else 0)
        hv = X.key_hash(idw=key[0], ck=key[1])
        h = X.dm_home(hv, mask)
        while h in table and not (table[h][0] == X.dm_fp(hv) and (trust_fingerprint or table[h][2] == key)):
            h = (h + 1) & mask
        if h not in table:
            table[h] = (X.dm_fp(hv), i, key)
            segs[h] = []
        segs[h].append(i)
    return sorted((pk[0], pk) for pk in segs.values()), set(table)


@pytest.mark.parametrize("kind", ["same_hash", "same_fp", "same_home"])
def test_demux_cases_need_the_key_comparison_and_the_wrap(kind):
    """A table that confirms on the full key gives segments_ref's segments on the constructed keys; one that trusts
    the fingerprint does not (same_hash, same_fp); same_home's run crosses the table's end."""
    k = 65
    rng = np.random.default_rng(k)
    which = np.repeat(np.arange(k), rng.integers(1, 6, k))
    rng.shuffle(which)
    n = len(which)
    mask = X.dm_table_slots(n) - 1
    status = np.ones(n, np.int8)
    idw, fields = np.zeros(k, np.uint64), A.DEMUX_CONN_KEY
    if kind == "same_hash":
        (idw, ck), fields = X.same_hash(k), A.DEMUX_ID | A.DEMUX_CONN_KEY
    elif kind == "same_fp":
        ck = X.same_fp(k, [(mask - 1 + j // 2) & mask for j in range(k)], mask)
    else:
        ck = X.same_home(k, mask - 1, mask)
    want = D.segments_ref(status, np.zeros(n, np.uint8), fields, idw[which].view(np.uint8), None, ck[which], None)[0]
    got, used = demux_model(status, fields, idw[which], ck[which])
    assert got == want and len(used) == k
    bad, used_bad = demux_model(status, fields, idw[which], ck[which], trust_fingerprint=True)
    if kind == "same_home":  # k different fingerprints: nothing to confuse, but one run of k entries from T - 2
        assert bad == want and used == {(mask - 1 + j) & mask for j in range(k)} and {mask, 0} <= used
    else:
        assert bad != want and len(used_bad) < k, "tests/collide.py: the constructed keys no longer share a fingerprint"


def aggregator_model(rows, drop_when_taken=False):
    """rsk_tile_dev.h's tile_count_rows for one tile without the leader rounds: every item claims its row's entry
    from the row's home on, or adds to it -- or is dropped when its home entry is another row's, the mutant."""
    tab_row, tab_cnt = np.full(X.AGG_SLOTS, -1, np.int64), np.zeros(X.AGG_SLOTS, np.int64)
    steps = 0
    for r, s in zip(rows.tolist(), X.agg_home(rows).tolist()):
        while tab_row[s] not in (-1, r):
            if drop_when_taken:
                s = -1
                break
            s = (s + 1) & (X.AGG_SLOTS - 1)
            steps += 1
        if s >= 0:
            tab_row[s] = r
            tab_cnt[s] += 1
    return dict(zip(tab_row[tab_row >= 0].tolist(), tab_cnt[tab_row >= 0].tolist())), steps


@pytest.mark.parametrize("pattern", ["distinct", "thrice", "half_one_row"])
def test_aggregator_cases_need_the_probe(pattern):
    """The rows of tests/conv_ref.band_packets fill one run of the LDS table across its end: the model counts them
    exactly after about a million probe steps for 2048 distinct rows; a table that drops an item whose home entry is
    taken loses counts on every pattern."""
    from tests import conv_ref as V

    rows = V.band_packets(V.band_rows(), 2048, pattern).astype(np.int64)
    want = dict(zip(*[a.tolist() for a in np.unique(rows, return_counts=True)]))
    got, steps = aggregator_model(rows)
    assert got == want
    assert pattern != "distinct" or steps > 1_000_000
    assert aggregator_model(rows, drop_when_taken=True)[0] != want
