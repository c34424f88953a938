"""TEST INFRASTRUCTURE: keys built to collide in the library's hash tables, and the structural contract of
the conn / conv index.

Every hash of the library is a bijection on 64 bits up to the final cut (splitmix64's finaliser, odd multipliers,
xor-shifts), so a key with a chosen hash value comes from running the hash backwards: no search, no luck.

  restatements   conn_slots / conn_mix / conn_home (rsock_amd/csrc/rsk_conn.h), the demux's key_hash, table home
                 and LDS home (rsk_demux.hip), the row aggregator's home (rsk_tile_dev.h).  tests/test_collide.py
                 compares their constants with the sources' text, so a change of a hash fails there by name.
  constructors   keys_at / ids_at / tuples_at / convs_at for the index, the pick's group entries, the offers hash
                 and the client's conv-only table; same_hash / same_fp / same_home / ids_same_fp_home /
                 epoch_keys for the demux; rows_in_band for the aggregator.
  index_invariant  rsk_conn.h's contract on an index as a call left it.

A `home` of the index family is a 21-bit number H: bits 32..52 of the hash.  A table of S entries (S <= 2^21, the
largest index there is) probes from H & (S - 1), so one H places a key in every table at once: H = WIDE - 3 is
entry S - 3 of the index, of the create calls' dedup table and of the offers table, whatever their sizes."""
from __future__ import annotations

import numpy as np

M64 = 2**64 - 1
GOLDEN = 0x9E3779B97F4A7C15
WIDE = 1 << 21  # homes are taken modulo the largest index (rsk_conn.h: capacity <= 2^20, slots <= 2^21)
EMPTY = 0xFFFFFFFF
LIVE = 1  # RSK_CONN_LIVE / RSK_CONV_LIVE

MIX_M1, MIX_M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MIX_SHIFTS = (30, 27, 31)

# rsk_demux.hip's key_hash: multipliers of (ep | xf << 32), id, conn key, (conv | dst << 32); then the finaliser
DM_C1, DM_C2, DM_C3, DM_C4 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xD6E8FEB86659FD93
DM_FIN_MUL = 0xBF58476D1CE4E5B9
DM_FIN_SHIFTS = (31, 29)
DM_LDS_SHIFT = 40
DM_LDS_SLOTS = 1024  # kLtab = 2 * kInsTile
DM_INS_TILE = 512

# rsk_tile_dev.h's RowAgg of the 2048-item tiles (PER = 8): kSlots = 2 * 8 * 256
AGG_MUL = 0x9E3779B1
AGG_SLOTS = 4096


def inv64(a):
    return pow(a, -1, 1 << 64)


def unxs(x, s):
    """The inverse of x ^= x >> s on 64 bits."""
    y = x
    for _ in range(64 // s + 1):
        y = x ^ (y >> s)
    return y


# ---- the index family --------------------------------------------------------------------------------------------
def conn_slots(capacity):
    s = 4
    while s < 2 * capacity:
        s <<= 1
    return s


def conn_mix(x):
    x ^= x >> 30
    x = x * MIX_M1 & M64
    x ^= x >> 27
    x = x * MIX_M2 & M64
    return x ^ (x >> 31)


def unmix(x):
    x = unxs(x, 31) * inv64(MIX_M2) & M64
    x = unxs(x, 27) * inv64(MIX_M1) & M64
    return unxs(x, 30)


def conn_home(key, idw, slots):
    return (conn_mix(key ^ conn_mix((idw + GOLDEN) & M64)) >> 32) & (slots - 1)


def group_home(idw, capacity):
    """conn_home(0, id, conn_slots(capacity)): where the probe for an IdBuf's group entry starts."""
    return conn_home(0, idw, conn_slots(capacity))


def _hashes(home, k, salt):
    """k distinct 64-bit hash values whose bits 32..52 are `home` (taken modulo WIDE, so -3 is entry S - 3)."""
    j = np.arange(1, k + 1, dtype=object) + salt * 0x10000
    return [((int(x) * 0x9E3779B1) & 0xFFFFFFFF) | ((home % WIDE) << 32) | ((int(x) & 0x7FF) << 53) for x in j], j


def keys_at(home, k, idw=0, salt=0):
    """k distinct conn keys whose probe starts at `home` under the id word(s) `idw` (a scalar or k words)."""
    hv, _ = _hashes(home, k, salt)
    ids = np.broadcast_to(np.asarray(idw, np.uint64), (k,))
    return np.array([unmix(h) ^ conn_mix((int(i) + GOLDEN) & M64) for h, i in zip(hv, ids)], np.uint64)


def ids_at(home, k, salt=0, key=0):
    """k distinct id words under which `key` (a scalar or k keys) probes from `home`; key = 0: the ids whose group
    entry conn_home(0, id, .) is `home`."""
    hv, _ = _hashes(home, k, salt)
    keys = np.broadcast_to(np.asarray(key, np.uint64), (k,))
    return np.array([(unmix(unmix(h) ^ int(x)) - GOLDEN) & M64 for h, x in zip(hv, keys)], np.uint64)


def tuples_at(home, k, salt=0):
    """k distinct 4-tuples for the offers hash conn_home(src << 32 | dst, sp << 16 | dp, .): -> (src, dst, sp, dp)."""
    hv, j = _hashes(home, k, salt)
    ports = [(0x80000000 | (int(x) * 40503)) & 0xFFFFFFFF for x in j]
    tk = np.array([unmix(h) ^ conn_mix((p + GOLDEN) & M64) for h, p in zip(hv, ports)], np.uint64)
    ports = np.array(ports, np.uint64)
    return ((tk >> np.uint64(32)).astype(np.uint32), tk.astype(np.uint32),
            (ports >> np.uint64(16)).astype(np.uint16), ports.astype(np.uint16))


def _mix_np(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(MIX_M1)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(MIX_M2)
    return x ^ (x >> np.uint64(31))


_CONV_HOMES = {}  # slots -> the homes of the convs 1 .. limit - 1 (index 0 unused), grown as a search needs


def convs_at(home, k, slots):
    """The first k 32-bit convs (from 1) whose probe in a conv-only table of `slots` entries starts at `home`
    (modulo slots): a search, the key has 32 bits only."""
    limit = 1 << 20
    while True:
        h = _CONV_HOMES.get(slots)
        if h is None or len(h) < limit:
            with np.errstate(over="ignore"):
                c = np.arange(limit, dtype=np.uint64)
                h = ((_mix_np(c ^ np.uint64(conn_mix(GOLDEN))) >> np.uint64(32)) & np.uint64(slots - 1)).astype(np.uint32)
            h[0] = 0xFFFFFFFF
            _CONV_HOMES[slots] = h
        got = np.nonzero(h == np.uint32(home % slots))[0][:k]
        if len(got) == k or limit == 1 << 32:
            break
        limit <<= 2
    assert len(got) == k, f"tests/collide.py: only {len(got)} convs with home {home % slots} of {slots}"
    return got.astype(np.uint32)


# ---- the demux ---------------------------------------------------------------------------------------------------
def dm_fin(h):
    h ^= h >> DM_FIN_SHIFTS[0]
    h = h * DM_FIN_MUL & M64
    return h ^ (h >> DM_FIN_SHIFTS[1])


def dm_unfin(h):
    h = unxs(h, DM_FIN_SHIFTS[1]) * inv64(DM_FIN_MUL) & M64
    return unxs(h, DM_FIN_SHIFTS[0])


def key_hash(ep=0, idw=0, ck=0, conv=0, dst=0, xf=0):
    return dm_fin(((ep | xf << 32) * DM_C1 ^ idw * DM_C2 ^ ck * DM_C3 ^ (conv | dst << 32) * DM_C4) & M64)


def dm_table_slots(n):
    """T = max(64, the power of two >= 2n): the global key table of a batch of n packets."""
    t = 64
    while t < 2 * n:
        t <<= 1
    return t


def dm_home(hv, mask):
    return hv & mask


def dm_lds_home(hv):
    return (hv ^ hv >> DM_LDS_SHIFT) & (DM_LDS_SLOTS - 1)


def dm_fp(hv):
    return hv >> 32


def same_hash(k, salt=0):
    """k distinct (id word, conn key) pairs with id * C2 ^ ck * C3 equal: one 64-bit key_hash in every epoch, with
    any conv / dst (as long as those are equal too).  -> (ids uint64 [k], ckeys uint64 [k])"""
    t = conn_mix(salt + 12345)
    ids = np.array([conn_mix(j + 1 + salt * 0x10000) for j in range(k)], np.uint64)
    ck = np.array([((t ^ int(i) * DM_C2) & M64) * inv64(DM_C3) & M64 for i in ids], np.uint64)
    return ids, ck


def _dm_hashes(k, fps, homes, mask):
    """Hash values with fingerprint fps[j] and table home homes[j] under `mask` (the bits between vary with j)."""
    out = []
    for j in range(k):
        mid = ((j + 1) * (mask + 1)) & 0xFFFFFFFF  # distinct for j < 2^32 / T, and no bit of the home
        out.append((int(fps[j]) << 32) | mid | (int(homes[j]) & mask))
    return out


def ckeys_for(hashes, ep=0):
    """Conn keys (the only selected field) whose key_hash in epoch `ep` are `hashes`."""
    return np.array([((dm_unfin(h) ^ ep * DM_C1) & M64) * inv64(DM_C3) & M64 for h in hashes], np.uint64)


def same_fp(k, homes, mask, fp=0xC0111DE5, ep=0):
    """k conn keys of one fingerprint and the table homes `homes` (conn-key-only selection, epoch ep)."""
    return ckeys_for(_dm_hashes(k, [fp] * k, homes, mask), ep)


def same_home(k, home, mask, ep=0):
    """k conn keys of one table home and k different fingerprints."""
    return ckeys_for(_dm_hashes(k, [0x51000000 + 7919 * j for j in range(k)], [home] * k, mask), ep)


def epoch_keys(hv, epochs):
    """For each epoch e the conn key whose key_hash in THAT epoch is hv (conn-key-only selection)."""
    return np.array([int(ckeys_for([hv], e)[0]) for e in epochs], np.uint64)


def ids_same_fp_home(k, mask, fp=0x1DB0F5ED, home=None):
    """k distinct id words whose IdBuf-only key (GROUP_BARRIER's first pass: epoch 0, no other field) has one
    fingerprint and one table home."""
    home = mask - 1 if home is None else home
    return np.array([dm_unfin(h) * inv64(DM_C2) & M64 for h in _dm_hashes(k, [fp] * k, [home] * k, mask)], np.uint64)


# ---- the row aggregator ------------------------------------------------------------------------------------------
def agg_home(row):
    shift = 32 - (AGG_SLOTS.bit_length() - 1)
    return ((np.asarray(row, np.uint64) * np.uint64(AGG_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(shift)


def rows_in_band(capacity, lo, width):
    """The rows below `capacity` whose aggregator home lies in [lo, lo + width) modulo AGG_SLOTS, ascending."""
    h = agg_home(np.arange(capacity))
    return np.nonzero(((h.astype(np.int64) - lo) % AGG_SLOTS) < width)[0].astype(np.uint32)


# ---- rsk_conn.h's contract ---------------------------------------------------------------------------------------
def homes_np(key_words, id_words, slots):
    """conn_home over arrays."""
    with np.errstate(over="ignore"):
        k = np.asarray(key_words, np.uint64) ^ _mix_np(np.asarray(id_words, np.uint64) + np.uint64(GOLDEN))
        return ((_mix_np(k) >> np.uint64(32)) & np.uint64(slots - 1)).astype(np.int64)


def linear_insert(slots, homes):
    """The occupied entries a sequential linear-probing insert of keys with these homes leaves.  The set does not
    depend on the insertion order: walking the entries in order with the number of keys still looking for a place,
    an entry is taken iff a key is waiting when the walk reaches it (twice round, so the wrap carries over)."""
    c = np.tile(np.bincount(np.asarray(homes, np.int64), minlength=slots), 2)
    s = np.cumsum(c - 1)
    waiting = s - np.minimum(0, np.minimum.accumulate(s))  # after each entry
    before = np.concatenate([[0], waiting[:-1]])
    return (before + c > 0)[slots:]


def index_invariant(index, capacity, state, key_words, id_words=None, by_id=False, live=None, what=""):
    """rsk_conn.h on an index as a call left it: every entry names a LIVE row of the table, no two entries hold one
    key, every LIVE key has an entry, which names its lowest LIVE row and has no free entry between the key's home
    and itself, and the occupied entries are those of a sequential insert.  `live`: the rows the index has to hold
    when they are not the LIVE rows of `state` (a conv close with HOLD forgets rows that stay LIVE).
    -> the number of occupied entries."""
    slots = conn_slots(capacity)
    index = np.asarray(index).view(np.uint32).ravel()
    assert len(index) == slots, (what, "the index has conn_slots(capacity) words", len(index), slots)
    live = (np.asarray(state) & LIVE) != 0 if live is None else np.asarray(live, bool)
    key_words = np.asarray(key_words).astype(np.uint64)
    idw = np.asarray(id_words, np.uint64) if by_id else np.zeros(capacity, np.uint64)
    free = index == EMPTY
    occ = np.nonzero(~free)[0]
    rows = index[occ].astype(np.int64)
    assert bool((rows < capacity).all()), (what, "an entry names no row of the table", rows[rows >= capacity][:4])
    assert bool(live[rows].all()), (what, "an entry names a row that is not LIVE", rows[~live[rows]][:4])
    # the entries' keys, sorted by (id word, key); no two equal
    o = np.lexsort((key_words[rows], idw[rows]))
    e_id, e_key, entry, held = idw[rows][o], key_words[rows][o], occ[o], rows[o]
    assert not bool(((e_id[1:] == e_id[:-1]) & (e_key[1:] == e_key[:-1])).any()), (what, "two entries hold one key")
    # the LIVE keys in the same order, each with its lowest LIVE row
    lr = np.nonzero(live)[0]
    o = np.lexsort((lr, key_words[lr], idw[lr]))
    l_id, l_key, lr = idw[lr][o], key_words[lr][o], lr[o]
    first = np.concatenate([[True], (l_id[1:] != l_id[:-1]) | (l_key[1:] != l_key[:-1])]) if len(lr) else np.zeros(0, bool)
    l_id, l_key, lowest = l_id[first], l_key[first], lr[first]
    assert len(entry) >= len(lowest), (what, "a LIVE key has no entry", len(entry), len(lowest))
    assert len(entry) == len(lowest) and np.array_equal(e_id, l_id) and np.array_equal(e_key, l_key), \
        (what, "the entries' keys are not the LIVE keys")
    assert np.array_equal(held, lowest), (what, "an entry is not its key's lowest LIVE row", np.nonzero(held != lowest)[0][:4])
    keys = np.stack([l_id, l_key], axis=1)
    home = homes_np(keys[:, 1], keys[:, 0], slots)
    span = (entry - home) & (slots - 1)
    nfree = np.concatenate([[0], np.cumsum(np.tile(free, 2))])
    gap = nfree[home + span] - nfree[home]
    assert bool((gap == 0).all()), (what, "a free entry between a key's home and its entry", keys[gap != 0][:2])
    want = linear_insert(slots, home)
    assert np.array_equal(~free, want), (what, "occupied entries differ from a sequential insert's",
                                         np.nonzero(~free != want)[0][:8])
    return len(occ)


def run_of(taken, home, length, what="the constructed keys"):
    """The taken entries of a table (a bool per entry) are exactly `length` consecutive ones from `home`, wrapping."""
    taken = np.asarray(taken, bool)
    slots = len(taken)
    want = np.zeros(slots, bool)
    want[(home % slots + np.arange(length)) & (slots - 1)] = True
    assert np.array_equal(taken, want), (f"tests/collide.py: {what} do not share one run", home % slots, length,
                                         np.nonzero(taken != want)[0][:8])


def one_run(index, home, length):
    """The occupied entries of a conn / conv index are one run of `length` from `home`: the proof, read back from
    the index a twin or the device built, that a constructed cluster is one."""
    run_of(np.asarray(index).view(np.uint32).ravel() != EMPTY, home, length)
