// rsk_host.cpp — host-side batch helpers of the header-only path (include/rsk_codec.h): staging
// the 32-B decode slots of received frames and assembling frames from encoded header slots and
// payloads, each over contiguous shards on std::threads; and the host twins of the payload delivery
// (rsk_deliver_host), of the checksum verification (rsk_verify_wire_host) and of the connection table
// (rsk_conn_*_host) with its send pick (rsk_conn_pick_*host), its control packets and keepalive timer (rsk_control_host,
// rsk_keepalive_flush_host), its close (rsk_conn_close_host), of the conv table (rsk_conv_*_host) and of the tuple pool (rsk_pool_*_host); the single-frame slot staging, the capture filter's text form and the connection
// keys.  Pure host code (no HIP calls).
#include <atomic>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rsk_codec.h"
#include "rsk_conn.h"
#include "rsk_conn_create.h"
#include "rsk_conv_create.h"
#include "rsk_pick.h"
#include "rsk_pool.h"

namespace {

template <typename F>
void for_shards(uint32_t n, int nthreads, F f) {
    if (nthreads <= 1 || n < 4096) {
        f(0u, n);
        return;
    }
    std::vector<std::thread> ts;
    const uint32_t per = (n + (uint32_t)nthreads - 1) / (uint32_t)nthreads;
    for (uint32_t lo = 0; lo < n; lo += per) ts.emplace_back(f, lo, lo + per < n ? lo + per : n);
    for (auto &t : ts) t.join();
}

}  // namespace

extern "C" int rsk_stage_decode_headers(uint32_t n, const uint8_t *arena, const uint64_t *frame_off,
                                        const uint16_t *frame_len, uint8_t *slots, int nthreads) {
    if (n && (!arena || !frame_off || !frame_len || !slots)) return RSK_EINVAL;
    for_shards(n, nthreads, [=](uint32_t lo, uint32_t hi) {
        for (uint32_t i = lo; i < hi; ++i)
            rsk_stage_decode_header(arena + frame_off[i], (int)frame_len[i], slots + 32ull * i);
    });
    return RSK_OK;
}

extern "C" int rsk_assemble_frames(uint32_t n, const uint8_t *hdr, const int32_t *status, const uint8_t *payload_arena,
                                   const uint64_t *pay_off, uint8_t *frame_arena, const uint64_t *frame_off,
                                   int nthreads) {
    if (n && (!hdr || !status || !payload_arena || !pay_off || !frame_arena || !frame_off)) return RSK_EINVAL;
    for_shards(n, nthreads, [=](uint32_t lo, uint32_t hi) {
        for (uint32_t i = lo; i < hi; ++i) {
            const int32_t st = status[i];
            if (st <= 0) continue;
            uint8_t *f = frame_arena + frame_off[i];
            std::memcpy(f, hdr + 32ull * i, RSK_HEAD_SIZE);                                   // RConn.cpp:101-103
            std::memcpy(f + RSK_HEAD_SIZE, payload_arena + pay_off[i], (size_t)(st - RSK_HEAD_SIZE));  // :104
        }
    });
    return RSK_OK;
}

// rsk_deliver_batch on host pointers: the copy SConn::OnRecv (server/SConn.cpp:77-89) and
// ClientGroup::send2Origin (client/ClientGroup.cpp:82-96) make per packet, into one dense arena.  The
// offsets are one serial prefix sum; the copies run over contiguous shards of positions.
extern "C" int rsk_deliver_host(uint32_t n, const rsk_deliver_in *in, const rsk_deliver_out *out, int nthreads) {
    if (!in || !out || !out->out_off) return RSK_EINVAL;
    const uint32_t al = out->align;
    if (al == 0u || al > 128u || (al & (al - 1u))) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(out->out_arena) & 15u) return RSK_EINVAL;
    if ((in->order == nullptr) != (in->n_order == nullptr)) return RSK_EINVAL;
    if (n && (!in->base_off || !in->pay_off || !in->pay_len || !in->status)) return RSK_EINVAL;
    if (n && out->out_arena && !in->arena) return RSK_EINVAL;
    if (n > (1u << 30)) return RSK_EINVAL;
    const uint32_t m = in->order ? (*in->n_order < n ? *in->n_order : n) : n;
    // packet of position k, or n when the position carries no bytes
    auto index = [=](uint32_t k) -> uint32_t {
        const uint32_t i = in->order ? in->order[k] : k;
        return i < n && in->status[i] == RSK_RECV_VALID ? i : n;
    };
    uint64_t *off = out->out_off;
    uint64_t run = 0;
    for (uint32_t k = 0; k < m; ++k) {
        off[k] = run;
        const uint32_t i = index(k);
        if (i < n) run += ((uint64_t)in->pay_len[i] + al - 1u) & ~(uint64_t)(al - 1u);
    }
    for (uint32_t k = m; k <= n; ++k) off[k] = run;
    if (out->total) *out->total = run;
    if (!out->out_arena) return RSK_OK;
    uint8_t *dst = out->out_arena;
    const uint64_t cap = out->out_cap;
    for_shards(m, nthreads, [=](uint32_t lo, uint32_t hi) {
        for (uint32_t k = lo; k < hi; ++k) {
            const uint64_t r = off[k + 1] - off[k];
            if (r == 0 || off[k + 1] > cap) continue;  // nothing to write, or cut by out_cap: not written at all
            const uint32_t i = index(k);
            const size_t len = in->pay_len[i];
            const uint8_t *src = in->arena + in->base_off[i] + (in->inner_off ? in->inner_off[i] : 0u) + in->pay_off[i];
            std::memcpy(dst + off[k], src, len);  // RConn.cpp:64-85's pointer, SConn.cpp:80's memcpy
            std::memset(dst + off[k] + len, 0, (size_t)r - len);
        }
    });
    return RSK_OK;
}

namespace {

uint32_t fold16(uint64_t s) {
    while (s >> 16) s = (s & 0xffffu) + (s >> 16);
    return (uint32_t)s;
}

// Ones'-complement sum of the len bytes at p as big-endian halfwords (an odd last byte is the high
// byte), folded to 16 bits.  Sums little-endian 32-bit words from p on -- the packet's halfwords
// byte-swapped -- and swaps the folded result once (RFC 1071 §2(B)).
uint32_t sum_be16(const uint8_t *p, size_t len) {
    uint64_t s = 0;
    size_t k = 0;
    for (; k + 4 <= len; k += 4) {
        uint32_t w;
        std::memcpy(&w, p + k, 4);
        s += w;
    }
    uint32_t tail = 0;
    std::memcpy(&tail, p + k, len - k);
    const uint32_t f = fold16(s + tail);
    return ((f & 0xffu) << 8) | (f >> 8);
}

// RSK_CSUM_* bits of one captured packet (the rule of rsk_verify_wire_batch, include/rsk_codec.h)
uint32_t verify_one(const uint8_t *p, uint32_t c, uint32_t L) {
    if (L == 14 && !(c >= 14 && p[12] == 0x08 && p[13] == 0x00)) return 0;
    if (L == 4 && !(c >= 4 && p[0] == 2 && p[1] == 0 && p[2] == 0 && p[3] == 0)) return 0;
    if (c < L + 20) return 0;
    const uint8_t *ip = p + L;
    const uint32_t ihl = ip[0] & 15u, H = 4 * ihl;
    if ((ip[0] >> 4) != 4 || ihl < 5 || c < L + H) return 0;
    uint32_t f = RSK_CSUM_IP_CHECKED;
    if (sum_be16(ip, H) == 0xffffu) f |= RSK_CSUM_IP_OK;
    const uint32_t tot = ((uint32_t)ip[2] << 8) | ip[3], frag = ((uint32_t)ip[6] << 8) | ip[7];
    if (ip[9] != 6 || (frag & 0x3fffu) || tot < H + 20) return f;
    if (L + tot > c) return f | RSK_CSUM_TCP_TRUNC;
    const uint32_t T = tot - H;
    f |= RSK_CSUM_TCP_CHECKED;
    if (fold16((uint64_t)sum_be16(ip + 12, 8) + 6u + T + sum_be16(ip + H, T)) == 0xffffu) f |= RSK_CSUM_TCP_OK;
    return f;
}

}  // namespace

// rsk_verify_wire_batch on host pointers, over contiguous shards of packets.
extern "C" int rsk_verify_wire_host(uint32_t n, const rsk_verify_in *in, int datalink, const rsk_verify_out *out,
                                    int nthreads) {
    if (!in || !out) return RSK_EINVAL;
    if (datalink != RSK_DLT_NULL && datalink != RSK_DLT_EN10MB && datalink != RSK_DLT_RAW) return RSK_EINVAL;
    if (out->status_out && !in->status) return RSK_EINVAL;
    if (n && (!in->cap_arena || !in->cap_off || !in->cap_len || !out->csum)) return RSK_EINVAL;
    const uint32_t L = datalink == RSK_DLT_EN10MB ? 14u : datalink == RSK_DLT_NULL ? 4u : 0u;
    std::atomic<uint32_t> bad_total{0};
    std::atomic<uint32_t> *bt = &bad_total;
    const rsk_verify_in a = *in;
    const rsk_verify_out o = *out;
    for_shards(n, nthreads, [=](uint32_t lo, uint32_t hi) {
        uint32_t nb = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            const int8_t st = a.status ? a.status[i] : (int8_t)RSK_RECV_VALID;
            const uint32_t f = st == RSK_RECV_VALID ? verify_one(a.cap_arena + a.cap_off[i], a.cap_len[i], L) : 0u;
            const bool bad = ((f & RSK_CSUM_IP_CHECKED) && !(f & RSK_CSUM_IP_OK)) ||
                             ((f & RSK_CSUM_TCP_CHECKED) && !(f & RSK_CSUM_TCP_OK));
            o.csum[i] = (uint8_t)f;
            if (o.status_out) o.status_out[i] = bad ? (int8_t)RSK_RECV_DROP : st;
            nb += bad;
        }
        bt->fetch_add(nb, std::memory_order_relaxed);
    });
    if (out->n_bad) *out->n_bad = bad_total.load();
    return RSK_OK;
}

// ---- connection table (rsk_conn_table): the host twins; hash and probe rule in rsk_conn.h -----------
namespace {

uint64_t load64(const uint8_t *p) {
    uint64_t v;
    std::memcpy(&v, p, 8);
    return v;
}

struct HostConnTab {
    const rsk_conn_table *t;
    uint32_t entry(uint32_t s) const { return t->index[s]; }
    uint64_t key(uint32_t row) const { return t->conn_key[row]; }
    uint64_t id(uint32_t row) const { return load64(t->id + 8ull * row); }
};

bool conn_tab_ok(const rsk_conn_table *t) {
    return t && !(t->flags & ~RSK_CONN_BY_ID) && t->capacity >= 1u && t->capacity <= RSK_CONN_MAX_ROWS;
}
// what a lookup reads
bool conn_tab_lookup_ok(const rsk_conn_table *t) {
    return conn_tab_ok(t) && t->conn_key && t->index && (!(t->flags & RSK_CONN_BY_ID) || t->id);
}

// The index of any table whose accessor T gives key(row) and id(row): rows in increasing order, so the
// first row of a key takes its entry and every later one is a duplicate.
template <typename T>
void index_build_host(const T &h, uint32_t *index, const uint8_t *state, uint32_t capacity, bool by_id, uint32_t *n_dup) {
    const uint32_t slots = rsk::conn_slots(capacity);
    std::memset(index, 0xFF, 4ull * slots);
    uint32_t dup = 0;
    for (uint32_t r = 0; r < capacity; ++r) {
        if (!(state[r] & RSK_CONN_LIVE)) continue;
        const uint64_t key = h.key(r), id = by_id ? h.id(r) : 0ull;
        for (uint32_t s = rsk::conn_home(key, id, slots);; s = rsk::conn_next(s, slots)) {
            const uint32_t e = index[s];
            if (e == rsk::kConnEmpty) { index[s] = r; break; }
            if (h.key(e) == key && (!by_id || h.id(e) == id)) { ++dup; break; }
        }
    }
    if (n_dup) *n_dup = dup;
}

}  // namespace

extern "C" uint64_t rsk_conn_index_bytes(uint32_t capacity, uint32_t flags) {
    if ((flags & ~RSK_CONN_BY_ID) || capacity < 1u || capacity > RSK_CONN_MAX_ROWS) return 0;
    return 4ull * rsk::conn_slots(capacity);
}

extern "C" int rsk_conn_index_build_host(const rsk_conn_table *t, uint32_t *n_dup, int /*nthreads*/) {
    if (!conn_tab_lookup_ok(t) || !t->state) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(t->index) & 15u) return RSK_EINVAL;
    index_build_host(HostConnTab{t}, t->index, t->state, t->capacity, (t->flags & RSK_CONN_BY_ID) != 0, n_dup);
    return RSK_OK;
}

extern "C" int rsk_conn_resolve_host(const rsk_conn_table *t, uint32_t n, const rsk_conn_resolve_in *in,
                                     const rsk_conn_resolve_out *out, int nthreads) {
    if (!in || !out || !conn_tab_lookup_ok(t)) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0;
    if (n && (!in->status || !in->conn_key || !out->conn || (by_id && !in->id))) return RSK_EINVAL;
    std::atomic<uint32_t> miss_total{0};
    std::atomic<uint32_t> *mt = &miss_total;
    const rsk_conn_resolve_in a = *in;
    const rsk_conn_resolve_out o = *out;
    const HostConnTab h{t};
    const uint32_t cap = t->capacity;
    for_shards(n, nthreads, [=](uint32_t lo, uint32_t hi) {
        uint32_t nm = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            const bool look = a.status[i] == RSK_RECV_VALID && (!a.cmd || a.cmd[i] == RSK_CMD_DATA);
            uint32_t row = RSK_CONN_NONE;
            if (look) row = rsk::conn_lookup(h, cap, by_id, a.conn_key[i], by_id ? load64(a.id + 8ull * i) : 0ull);
            const bool miss = look && row == RSK_CONN_NONE;
            o.conn[i] = row;
            if (o.hit) o.hit[i] = row != RSK_CONN_NONE;
            if (o.miss) o.miss[i] = miss ? (int8_t)RSK_RECV_VALID : (int8_t)RSK_RECV_DROP;
            nm += miss;
        }
        mt->fetch_add(nm, std::memory_order_relaxed);
    });
    if (out->n_miss) *out->n_miss = miss_total.load();
    return RSK_OK;
}

extern "C" int rsk_conn_expand_host(const rsk_conn_table *t, uint32_t n, const uint32_t *conn,
                                    const rsk_conn_expand_out *out, int nthreads) {
    if (!out || !conn_tab_ok(t) || !t->state) return RSK_EINVAL;
    if ((out->src && !t->src) || (out->dst && !t->dst) || (out->sp && !t->sp) || (out->dp && !t->dp) ||
        (out->ack && !t->ack) || (out->flag && !t->flag) || (out->conn_key && !t->conn_key) || (out->id && !t->id))
        return RSK_EINVAL;
    if (n && (!conn || !out->ok)) return RSK_EINVAL;
    std::atomic<uint32_t> bad_total{0};
    std::atomic<uint32_t> *bt = &bad_total;
    const rsk_conn_expand_out o = *out;
    const rsk_conn_table tab = *t;
    for_shards(n, nthreads, [=](uint32_t lo, uint32_t hi) {
        constexpr uint8_t kUp = RSK_CONN_LIVE | RSK_CONN_ALIVE;
        uint32_t nb = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t r = conn[i];
            const bool ok = r < tab.capacity && (tab.state[r] & kUp) == kUp;
            if (o.src) o.src[i] = ok ? tab.src[r] : 0u;
            if (o.dst) o.dst[i] = ok ? tab.dst[r] : 0u;
            if (o.sp) o.sp[i] = ok ? tab.sp[r] : (uint16_t)0;
            if (o.dp) o.dp[i] = ok ? tab.dp[r] : (uint16_t)0;
            if (o.ack) o.ack[i] = ok ? tab.ack[r] : 0u;
            if (o.flag) o.flag[i] = ok ? tab.flag[r] : (uint8_t)0;
            if (o.conn_key) o.conn_key[i] = ok ? tab.conn_key[r] : 0ull;
            if (o.id) {
                if (ok) std::memcpy(o.id + 8ull * i, tab.id + 8ull * r, 8);
                else std::memset(o.id + 8ull * i, 0, 8);
            }
            o.ok[i] = ok;
            nb += !ok;
        }
        bt->fetch_add(nb, std::memory_order_relaxed);
    });
    if (out->n_bad) *out->n_bad = bad_total.load();
    return RSK_OK;
}

// ---- the send pick (rsk_conn_pick_build / rsk_conn_pick_batch): the host twins; layout in rsk_pick.h ----
namespace {

struct HostPick {
    const uint32_t *w;
    rsk::PickLayout l;
    uint32_t word(uint32_t i) const { return w[i]; }
    rsk::PickGroup group(uint32_t s) const {
        rsk::PickGroup g;
        std::memcpy(&g, w + l.group + 4ull * s, sizeof g);
        return g;
    }
    uint32_t cand(uint32_t i) const { return w[l.cand + i]; }
    uint32_t pos(uint32_t r) const { return w[l.pos + r]; }
};

bool pick_tab_ok(const rsk_conn_table *t) {
    return conn_tab_ok(t) && (!(t->flags & RSK_CONN_BY_ID) || t->id);
}

}  // namespace

extern "C" uint64_t rsk_conn_pick_bytes(uint32_t capacity, uint32_t flags) {
    if ((flags & ~RSK_CONN_BY_ID) || capacity < 1u || capacity > RSK_CONN_MAX_ROWS) return 0;
    return 4ull * rsk::pick_layout(capacity, (flags & RSK_CONN_BY_ID) != 0).words;
}

extern "C" int rsk_conn_pick_build_host(const rsk_conn_table *t, uint32_t *pick, uint32_t *counts, int /*nthreads*/) {
    constexpr uint8_t kUp = RSK_CONN_LIVE | RSK_CONN_ALIVE;
    if (!pick_tab_ok(t) || !t->state || !pick) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(pick) & 15u) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0;
    const uint32_t cap = t->capacity, slots = rsk::conn_slots(cap);
    const rsk::PickLayout l = rsk::pick_layout(cap, by_id);
    std::memset(pick, 0, 4ull * rsk::kPickHdr);
    std::memset(pick + l.cand, 0xFF, 4ull * (l.group - l.cand));  // cand, pos and lead: kConnEmpty
    std::memset(pick + l.group, 0, 4ull * (l.words - l.group));
    rsk::PickGroup *grp = reinterpret_cast<rsk::PickGroup *>(pick + l.group);  // 16-B aligned with pick
    uint32_t *lead = pick + l.lead;
    auto up = [&](uint32_t r) { return (t->state[r] & kUp) == kUp; };
    // the entry of a candidate row's IdBuf (taken by the first pass below)
    auto slot_of = [&](uint64_t id) {
        uint32_t s = rsk::conn_home(0ull, id, slots);
        while (lead[s] != rsk::kConnEmpty && grp[s].id != id) s = rsk::conn_next(s, slots);
        return s;
    };
    uint32_t total = 0, groups = 0;
    if (by_id) {
        for (uint32_t r = 0; r < cap; ++r) {  // the groups and their counts
            if (!up(r)) continue;
            const uint64_t id = load64(t->id + 8ull * r);
            const uint32_t s = slot_of(id);
            if (lead[s] == rsk::kConnEmpty) { lead[s] = r; grp[s].id = id; }
            ++grp[s].cnt;
        }
        for (uint32_t r = 0; r < cap; ++r) {  // their offsets, in the order of their lowest rows
            if (!up(r)) continue;
            const uint32_t s = slot_of(load64(t->id + 8ull * r));
            if (lead[s] != r) continue;
            grp[s].off = total;
            total += grp[s].cnt;
            grp[s].cnt = 0;  // counts up again as the rows take their positions
            ++groups;
        }
    }
    for (uint32_t r = 0; r < cap; ++r) {
        if (!up(r)) continue;
        uint32_t off = 0, p;
        if (by_id) {
            rsk::PickGroup &g = grp[slot_of(load64(t->id + 8ull * r))];
            off = g.off;
            p = g.cnt++;
        } else {
            p = total++;
        }
        pick[l.pos + r] = p;
        pick[l.cand + off + p] = r;
    }
    if (!by_id) groups = total != 0u;
    pick[0] = total;
    pick[1] = groups;
    if (counts) { counts[0] = groups; counts[1] = total; }
    return RSK_OK;
}

extern "C" int rsk_conn_pick_host(const rsk_conn_table *t, const uint32_t *pick, uint32_t n, const rsk_conn_pick_in *in,
                                  const rsk_conn_pick_out *out, int nthreads) {
    if (!in || !out || !pick || !pick_tab_ok(t)) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(pick) & 15u) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0;
    if (in->avoid_key && (!t->conn_key || !t->index)) return RSK_EINVAL;
    if (n && (!out->conn || (by_id && !in->id))) return RSK_EINVAL;
    std::atomic<uint32_t> none_total{0};
    std::atomic<uint32_t> *nt = &none_total;
    const rsk_conn_pick_in a = *in;
    const rsk_conn_pick_out o = *out;
    const HostConnTab h{t};
    const uint32_t cap = t->capacity;
    const HostPick p{pick, rsk::pick_layout(cap, by_id)};
    for_shards(n, nthreads, [=](uint32_t lo, uint32_t hi) {
        uint32_t nn = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            if (a.len && a.len[i] <= 0) {  // not taken: nothing else of it is read
                o.conn[i] = RSK_CONN_NONE;
                continue;
            }
            const uint64_t id = by_id ? load64(a.id + 8ull * i) : 0ull;
            uint32_t off, m, row = RSK_CONN_NONE;
            if (rsk::pick_group(p, cap, by_id, id, off, m)) {
                const uint32_t d = a.draw ? a.draw[i] : (uint32_t)(rsk::pick_splitmix64_at(a.seed, i) >> 32);
                const uint64_t av = a.avoid_key ? a.avoid_key[i] : 0ull;
                uint32_t ap = rsk::kConnEmpty;
                if (av != 0ull) {
                    const uint32_t r = rsk::conn_lookup(h, cap, by_id, av, id);
                    if (r != rsk::kConnEmpty) ap = p.pos(r);
                }
                row = rsk::pick_row(p, cap, off, m, d, ap);
            }
            o.conn[i] = row;
            if (row == RSK_CONN_NONE) ++nn;
            else if (o.used) o.used[row] = 1;
        }
        nt->fetch_add(nn, std::memory_order_relaxed);
    });
    if (out->n_none) *out->n_none = none_total.load();
    return RSK_OK;
}

// ---- control packets and the keepalive timer (rsk_control_batch / rsk_keepalive_flush): the host twins ----
namespace {

bool ctl_msgs_any(const rsk_ctl_msgs &m) {
    return m.cmd || m.body || m.id || m.src || m.avoid_key || m.pay_off || m.pay_len;
}

void ctl_put_msg(const rsk_ctl_msgs &m, uint32_t k, uint8_t cmd, uint64_t body, const uint8_t *id, uint32_t src,
                 uint64_t avoid) {
    if (m.cmd) m.cmd[k] = cmd;
    if (m.body) m.body[k] = body;
    if (m.id) {
        if (id) std::memcpy(m.id + 8ull * k, id, 8);
        else std::memset(m.id + 8ull * k, 0, 8);
    }
    if (m.src) m.src[k] = src;
    if (m.avoid_key) m.avoid_key[k] = avoid;
    if (m.pay_off) m.pay_off[k] = 8ull * k;
    if (m.pay_len) m.pay_len[k] = 8;
}

}  // namespace

// Classification, body read and lookup per packet over shards; then one walk in packet order for the
// per-row effects, the counts and the message list.
extern "C" int rsk_control_host(const rsk_conn_table *t, uint32_t n, const rsk_control_in *in, const rsk_control_out *out,
                                int nthreads) {
    if (!in || !out || !conn_tab_lookup_ok(t)) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0;
    if (n && (!in->status || !in->cmd || !in->arena || !in->base_off || !in->pay_off || !in->pay_len || (by_id && !in->id)))
        return RSK_EINVAL;
    if ((in->tcp_sp == nullptr) != (in->tcp_dp == nullptr)) return RSK_EINVAL;
    if (in->miss && !in->conn_key) return RSK_EINVAL;
    const bool list = ctl_msgs_any(out->msgs);
    if (list && !out->msgs.n_msg) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    if (out->rst_first) std::memset(out->rst_first, 0xFF, 4ull * t->capacity);
    std::vector<uint8_t> kind(n);
    std::vector<uint64_t> arg(n);
    std::vector<uint32_t> conn(n);
    uint8_t *kd = kind.data();
    uint64_t *ag = arg.data();
    uint32_t *cn = conn.data();
    const rsk_control_in a = *in;
    const HostConnTab h{t};
    const uint32_t cap = t->capacity;
    const bool close_ok = in->tcp_sp && !by_id;
    for_shards(n, nthreads, [=](uint32_t lo, uint32_t hi) {
        for (uint32_t i = lo; i < hi; ++i) {
            uint8_t k = RSK_CTL_NONE;
            uint64_t v = 0;
            uint32_t row = RSK_CONN_NONE;
            if (a.status[i] == RSK_RECV_VALID) {
                const uint8_t cm = a.cmd[i];
                if (cm > 4u) {
                    k = RSK_CTL_UNKNOWN;
                } else if (cm != RSK_CMD_DATA) {
                    const uint32_t need = cm == RSK_CMD_CONV_RST ? 4u : 8u;
                    if (a.pay_len[i] < need) {
                        k = RSK_CTL_SHORT;
                    } else {
                        k = cm;  // RSK_CTL_CONV_RST .. RSK_CTL_KA_RESP are the cmd values
                        const uint8_t *p = a.arena + a.base_off[i] + (a.inner_off ? a.inner_off[i] : 0u) + a.pay_off[i];
                        if (need == 4u) {
                            uint32_t w;
                            std::memcpy(&w, p, 4);  // decode_uint32 (ConnReset.cpp:50)
                            v = w;
                        } else {
                            v = load64(p);  // KeyGenerator::DecodeKeySafe
                        }
                    }
                }
            } else if (a.status[i] == RSK_RECV_CLOSE && close_ok) {
                k = RSK_CTL_TCP_CLOSE;
                v = rsk_key_for_tcp(a.tcp_sp[i], a.tcp_dp[i]);
            }
            if (k >= RSK_CTL_NETCONN_RST && k <= RSK_CTL_TCP_CLOSE)
                row = rsk::conn_lookup(h, cap, by_id, v, by_id ? load64(a.id + 8ull * i) : 0ull);
            kd[i] = k;
            ag[i] = v;
            cn[i] = row;
        }
    });
    uint32_t n_msg = 0, n_ctl = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t k = kind[i];
        const uint32_t row = conn[i];
        n_ctl += k != RSK_CTL_NONE;
        if (out->kind) out->kind[i] = k;
        if (out->arg) out->arg[i] = arg[i];
        if (out->conn) out->conn[i] = row;
        if (row != RSK_CONN_NONE) {
            if (out->rst_first && (k == RSK_CTL_NETCONN_RST || k == RSK_CTL_TCP_CLOSE) && out->rst_first[row] == 0xFFFFFFFFu)
                out->rst_first[row] = i;
            if (out->ka_tries && k == RSK_CTL_KA_RESP) out->ka_tries[row] = RSK_KA_NONE;
        }
        const uint8_t *idp = in->id ? in->id + 8ull * i : nullptr;
        if (k == RSK_CTL_KA_REQ) {
            const bool hit = row != RSK_CONN_NONE;
            if (list) ctl_put_msg(out->msgs, n_msg, hit ? RSK_CMD_KEEP_ALIVE_RESP : RSK_CMD_NETCONN_RST, arg[i], idp, i,
                                  hit ? 0ull : arg[i]);
            ++n_msg;
        } else if (in->miss && in->miss[i] == RSK_RECV_VALID) {
            if (list) ctl_put_msg(out->msgs, n_msg, RSK_CMD_NETCONN_RST, in->conn_key[i], idp, i, in->conn_key[i]);
            ++n_msg;
        }
    }
    if (out->msgs.n_msg) *out->msgs.n_msg = n_msg;
    if (out->n_ctl) *out->n_ctl = n_ctl;
    return RSK_OK;
}

// Rows in order on the caller's thread (the lists are in row order; nthreads is taken for symmetry).
extern "C" int rsk_keepalive_flush_host(const rsk_conn_table *t, const rsk_keepalive *ka, const rsk_keepalive_out *out,
                                        int /*nthreads*/) {
    if (!ka || !out || !conn_tab_ok(t) || !t->state || !t->conn_key) return RSK_EINVAL;
    if (!ka->ka_tries || !ka->established_ms) return RSK_EINVAL;
    if (ka->max_retry < 1u || ka->max_retry > 254u) return RSK_EINVAL;
    const bool list = ctl_msgs_any(out->msgs);
    if ((list && !out->msgs.n_msg) || (out->dead_rows && !out->n_dead)) return RSK_EINVAL;
    uint32_t n_msg = 0, n_dead = 0;
    const int32_t delay = (int32_t)ka->request_delay_ms;
    for (uint32_t r = 0; r < t->capacity; ++r) {
        const uint8_t st = t->state[r];
        if (!(st & RSK_CONN_LIVE)) {  // removeInvalidRequest
            ka->ka_tries[r] = RSK_KA_NONE;
            continue;
        }
        if (!ka->online) continue;
        uint32_t tries = ka->ka_tries[r];
        const uint64_t est = ka->established_ms[r];
        // canSendRequest: `int df = timestampMs - conn->EstablishedTimeStampMs()`, truncation included
        if (!(st & RSK_CONN_NEW) && ka->now_ms > est && (int32_t)(uint32_t)(ka->now_ms - est) >= delay) {
            const bool had = tries != RSK_KA_NONE;
            tries = had ? (tries + 1u) & 0xFFu : 0u;
            if (!had || tries < ka->max_retry) {
                if (list) ctl_put_msg(out->msgs, n_msg, RSK_CMD_KEEP_ALIVE_REQ, t->conn_key[r], t->id ? t->id + 8ull * r : nullptr, r, 0ull);
                ++n_msg;
            }
        }
        if (tries != RSK_KA_NONE && tries >= ka->max_retry) {  // keep alive timeout
            tries = RSK_KA_NONE;
            if (out->dead_rows) out->dead_rows[n_dead] = r;
            ++n_dead;
        }
        ka->ka_tries[r] = (uint8_t)tries;
    }
    if (out->msgs.n_msg) *out->msgs.n_msg = n_msg;
    if (out->n_dead) *out->n_dead = n_dead;
    return RSK_OK;
}

// ---- conn close (rsk_conn_close_batch): the host twin; the pick update's layout and arithmetic in rsk_pick.h ----
extern "C" uint64_t rsk_conn_close_bytes(uint32_t capacity, uint32_t flags) {
    if ((flags & ~RSK_CONN_BY_ID) || capacity < 1u || capacity > RSK_CONN_MAX_ROWS) return 0;
    return 4ull * rsk::close_layout(capacity, (flags & RSK_CONN_BY_ID) != 0).words;
}

// The marks (list form: in `work`, as on the device), the two lists and the pick index from the state the call
// found, then the rows' state, and the conn index over the rows that stay when one was removed.
extern "C" int rsk_conn_close_host(const rsk_conn_table *t, const rsk_conn_rows *rows, const rsk_conn_close_in *in,
                                   const rsk_conn_close_out *out, int /*nthreads*/) {
    constexpr uint8_t kUp = RSK_CONN_LIVE | RSK_CONN_ALIVE, kGone = RSK_CONN_LIVE | RSK_CONN_ALIVE | RSK_CONN_NEW;
    if (!rows || !in || !out || !conn_tab_lookup_ok(t) || !t->state) return RSK_EINVAL;
    if (rows->state != t->state || !in->work) return RSK_EINVAL;
    const bool list = in->close_rows != nullptr, col = in->rst_first != nullptr;
    if ((in->flags & ~(RSK_CONN_CLOSE_REMOVE | RSK_CONN_CLOSE_SWEEP)) || (list && col) ||
        (!list && !col && !(in->flags & RSK_CONN_CLOSE_SWEEP)))
        return RSK_EINVAL;
    if (list && !in->n_close) return RSK_EINVAL;
    if ((out->marked_rows && !out->n_marked) || (out->closed_rows && !out->n_closed)) return RSK_EINVAL;
    if ((reinterpret_cast<uintptr_t>(t->index) | reinterpret_cast<uintptr_t>(in->work) | reinterpret_cast<uintptr_t>(out->pick)) & 15u)
        return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0;
    const bool remove = (in->flags & RSK_CONN_CLOSE_REMOVE) != 0, sweep = (in->flags & RSK_CONN_CLOSE_SWEEP) != 0;
    const uint32_t cap = t->capacity, c4 = (cap + 3u) & ~3u;
    const rsk::CloseLayout wl = rsk::close_layout(cap, by_id);
    uint32_t *work = static_cast<uint32_t *>(in->work);
    const uint8_t *mark = list ? static_cast<const uint8_t *>(in->work) : nullptr;
    if (list) {
        uint8_t *mk = static_cast<uint8_t *>(in->work);
        std::memset(mk, 0, 4ull * wl.k);
        const uint32_t m = *in->n_close < in->m_max ? *in->n_close : in->m_max;
        for (uint32_t j = 0; j < m; ++j)
            if (in->close_rows[j] < cap) mk[in->close_rows[j]] = 1;
    }
    auto marked = [&](uint32_t r) { return mark ? mark[r] != 0 : col ? in->rst_first[r] != 0xFFFFFFFFu : false; };
    auto next_state = [&](uint32_t r) {
        uint8_t st = rows->state[r];
        if (!(st & RSK_CONN_LIVE)) return st;
        const bool m = marked(r);
        if (m) st = (uint8_t)(st & ~RSK_CONN_ALIVE);
        if ((remove && m) || (sweep && !(st & RSK_CONN_ALIVE))) st = (uint8_t)(st & ~kGone);
        return st;
    };
    uint32_t n_marked = 0, n_closed = 0;
    for (uint32_t r = 0; r < cap; ++r) {
        const uint8_t d = (uint8_t)(rows->state[r] ^ next_state(r));
        if (d & RSK_CONN_ALIVE) {
            if (out->marked_rows) out->marked_rows[n_marked] = r;
            ++n_marked;
        }
        if (d & RSK_CONN_LIVE) {
            if (out->closed_rows) out->closed_rows[n_closed] = r;
            ++n_closed;
        }
    }
    if (out->pick && n_marked) {  // a row lost ALIVE: the candidates compacted in place (a new position is no later)
        uint32_t *pick = out->pick;
        const rsk::PickLayout pl = rsk::pick_layout(cap, by_id);
        const uint32_t tot0 = pick[0] < cap ? pick[0] : cap, kt = wl.tiles * rsk::kPickTile;
        uint32_t *K = work + wl.k;
        uint32_t total = 0;
        for (uint32_t j = 0; j < kt; ++j) {
            K[j] = total;
            if (j >= tot0) continue;
            const uint32_t r = pick[pl.cand + j];
            if (r >= cap) continue;
            if ((rows->state[r] & kUp) != kUp || marked(r)) {
                pick[pl.pos + r] = rsk::kConnEmpty;
                continue;
            }
            const uint32_t p = pick[pl.pos + r], o = p <= j ? j - p : rsk::kConnEmpty;  // the group's old offset
            pick[pl.cand + total] = r;
            pick[pl.pos + r] = !by_id ? total : o < cap && K[o] <= total ? total - K[o] : rsk::kConnEmpty;
            ++total;
        }
        for (uint32_t j = total; j < c4; ++j) pick[pl.cand + j] = rsk::kConnEmpty;
        auto k_at = [&](uint32_t j) { return j < kt ? K[j] : total; };
        uint32_t groups = pick[1];
        if (!by_id) groups = total != 0u;
        for (uint32_t s = 0; by_id && s < rsk::conn_slots(cap); ++s) {
            uint32_t *g = pick + pl.group + 4ull * s;  // {id lo, id hi, off, cnt}
            if (g[3] == 0u || g[2] >= cap || g[3] > cap - g[2]) continue;  // free, emptied before, or garbage
            const uint32_t k0 = k_at(g[2]), k1 = k_at(g[2] + g[3]);
            if (k1 > k0) {
                g[2] = k0;
                g[3] = k1 - k0;
            } else {
                g[2] = rsk::kPickGoneOff;
                g[3] = rsk::kPickGoneCnt;
                --groups;
            }
        }
        pick[0] = total;
        pick[1] = groups;
    }
    if (out->pick && out->pick_counts) {
        out->pick_counts[0] = out->pick[1];
        out->pick_counts[1] = out->pick[0];
    }
    if (n_marked || n_closed)
        for (uint32_t r = 0; r < cap; ++r) {
            const uint8_t ns = next_state(r);
            if (ns != rows->state[r]) rows->state[r] = ns;
        }
    if (n_closed) index_build_host(HostConnTab{t}, t->index, t->state, cap, by_id, nullptr);
    if (out->n_marked) *out->n_marked = n_marked;
    if (out->n_closed) *out->n_closed = n_closed;
    return RSK_OK;
}

// ---- conn create (rsk_conn_create_batch): the host twin; the argument rules and the row's seq / ack in
// rsk_conn_create.h ----
extern "C" uint64_t rsk_conn_create_bytes(uint32_t u_max, uint32_t m_max, uint32_t capacity, uint32_t flags) {
    if ((flags & ~RSK_CONN_BY_ID) || capacity < 1u || capacity > RSK_CONN_MAX_ROWS) return 0;
    if (u_max > rsk::kCreateMaxU || m_max == 0u || m_max > rsk::kCcMaxOffers) return 0;
    return 4ull * rsk::conn_create_layout(u_max, m_max, capacity).words;
}

namespace {

// The pick index over the state as it is, keeping the entry of every group that has candidates where it is: an
// IdBuf without one takes the first entry of its probe chain that is free or that rsk_conn_close_host left without
// candidates.  Every pick is what a fresh build gives; a walk over a garbage index is
// bounded and leaves the id without a group.
void pick_refresh_host(const rsk_conn_table *t, uint32_t *pick) {
    constexpr uint8_t kUp = RSK_CONN_LIVE | RSK_CONN_ALIVE;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0;
    const uint32_t cap = t->capacity, slots = rsk::conn_slots(cap), c4 = (cap + 3u) & ~3u;
    const rsk::PickLayout l = rsk::pick_layout(cap, by_id);
    std::memset(pick + l.cand, 0xFF, 4ull * 2u * c4);  // cand and pos
    uint32_t total = 0, groups = 0;
    if (!by_id) {
        for (uint32_t r = 0; r < cap; ++r)
            if ((t->state[r] & kUp) == kUp) {
                pick[l.pos + r] = total;
                pick[l.cand + total++] = r;
            }
        groups = total != 0u;
    } else {
        std::vector<uint32_t> cnt(slots, 0u), order, slot_of(cap, rsk::kConnEmpty);
        std::vector<uint8_t> mine(slots, 0);  // the entry was given to an IdBuf by this pass
        for (uint32_t r = 0; r < cap; ++r) {
            if ((t->state[r] & kUp) != kUp) continue;
            const uint64_t id = load64(t->id + 8ull * r);
            // the IdBuf's entry: one this pass gave it, or the one its candidates have; else the first entry of its
            // chain that is free or that a close left without candidates (whatever IdBuf that one holds: to every
            // pick an emptied group is one without an entry), so the entries in use stay bounded by the groups
            uint32_t s = rsk::conn_home(0ull, id, slots), found = rsk::kConnEmpty, take = rsk::kConnEmpty;
            for (uint32_t step = 0; step < slots; ++step, s = rsk::conn_next(s, slots)) {
                const uint32_t *g = pick + l.group + 4ull * s;
                if (g[3] == 0u) {  // free: the chain ends
                    if (take == rsk::kConnEmpty) take = s;
                    break;
                }
                uint64_t gid;
                std::memcpy(&gid, g, 8);
                const bool has = g[2] < cap && g[3] <= cap - g[2];
                if (gid == id && (mine[s] || has)) { found = s; break; }
                if (take == rsk::kConnEmpty && !mine[s] && g[2] == rsk::kPickGoneOff && g[3] == rsk::kPickGoneCnt) take = s;
            }
            if (found == rsk::kConnEmpty && take != rsk::kConnEmpty) {
                uint32_t *g = pick + l.group + 4ull * take;
                std::memcpy(g, &id, 8);
                g[2] = rsk::kPickTakenOff;
                g[3] = rsk::kPickGoneCnt;
                mine[take] = 1;
                found = take;
            }
            if (found == rsk::kConnEmpty) continue;
            if (cnt[found]++ == 0u) order.push_back(found);
            slot_of[r] = found;
        }
        for (uint32_t s = 0; s < slots; ++s) {  // entries whose group has no candidate (any more)
            uint32_t *g = pick + l.group + 4ull * s;
            if (g[3] != 0u && cnt[s] == 0u) { g[2] = rsk::kPickGoneOff; g[3] = rsk::kPickGoneCnt; }
        }
        for (uint32_t s : order) {  // in the order of the groups' lowest candidate rows
            uint32_t *g = pick + l.group + 4ull * s;
            g[2] = total;
            g[3] = 0u;
            total += cnt[s];
            ++groups;
        }
        for (uint32_t r = 0; r < cap; ++r) {
            if (slot_of[r] == rsk::kConnEmpty) continue;
            uint32_t *g = pick + l.group + 4ull * slot_of[r];
            pick[l.pos + r] = g[3];
            pick[l.cand + g[2] + g[3]++] = r;
        }
    }
    pick[0] = total;
    pick[1] = groups;
}

}  // namespace

// The walk of the header's rules in item order: the first arrivals of the considered packets (or the offers of
// the list form), each looking for its offer, take the vacant rows; then one pass over the batch for the
// packets that now resolve.  `work` is not used.
extern "C" int rsk_conn_create_host(const rsk_conn_table *t, const rsk_conn_create_rows *rows, uint32_t n,
                                    const rsk_conn_create_in *in, const rsk_conn_create_out *out, int /*nthreads*/) {
    if (!rsk::conn_create_args_ok(t, rows, n, in, out, false)) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONN_BY_ID) != 0, list = (in->flags & RSK_CONN_CREATE_LIST) != 0;
    const bool repeat = (in->flags & RSK_CONN_CREATE_REPEAT) != 0;
    const rsk_conn_offers &of = in->offers;
    const uint32_t cap = t->capacity, no = *of.n_offer < of.m_max ? *of.n_offer : of.m_max;
    const uint32_t m = of.m_max < cap ? of.m_max : cap;
    const HostConnTab h{t};
    typedef std::pair<uint64_t, uint64_t> K2;
    // items and their keys
    std::vector<uint32_t> items;
    if (list) {
        for (uint32_t o = 0; o < no; ++o) items.push_back(o);
    } else {
        for (uint32_t i = 0; i < n && items.size() < in->u_max; ++i)
            if (out->miss[i] == RSK_RECV_VALID) items.push_back(i);
    }
    auto item_key = [&](uint32_t x) {
        return list ? K2(of.conn_key[x], by_id ? load64(of.id + 8ull * x) : 0ull)
                    : K2(in->conn_key[x], by_id ? load64(in->id + 8ull * x) : 0ull);
    };
    std::map<std::pair<K2, uint64_t>, uint32_t> tuple_offer;  // column form: a tuple's lowest offer
    std::vector<uint8_t> taken(no, 0);
    if (!list)
        for (uint32_t o = 0; o < no; ++o) {
            tuple_offer.emplace(std::make_pair(K2(of.src[o], of.dst[o]), rsk::tuple_ports(of.sp[o], of.dp[o])), o);
            if (repeat && out->offer_row[o] != RSK_CONN_NONE) taken[o] = 1;
        }
    std::map<K2, uint32_t> seen;
    std::vector<uint32_t> got_item, got_offer;  // the offered keys, in first-arrival order
    uint32_t keys = 0;
    for (uint32_t x : items) {
        const K2 k = item_key(x);
        if (!seen.emplace(k, x).second) continue;
        ++keys;
        uint32_t o = RSK_CONN_NONE;
        if (list) {
            if (rsk::conn_lookup(h, cap, by_id, k.first, k.second) == rsk::kConnEmpty) o = x;
        } else {
            auto it = tuple_offer.find(std::make_pair(K2(in->src[x], in->dst[x]), rsk::tuple_ports(in->sp[x], in->dp[x])));
            if (it != tuple_offer.end() && !taken[it->second]) {
                o = it->second;
                taken[o] = 1;
            }
        }
        if (o == RSK_CONN_NONE) continue;
        got_item.push_back(x);
        got_offer.push_back(o);
    }
    if (list) keys = no;  // every offer is asked; the ones that repeat a key are refused too
    if (out->offer_row)
        for (uint32_t o = 0; o < no; ++o)
            if (!(repeat && out->offer_row[o] != RSK_CONN_NONE)) out->offer_row[o] = RSK_CONN_NONE;
    const uint32_t slots = rsk::conn_slots(cap);
    uint32_t n_new = 0, v = 0;
    for (size_t q = 0; q < got_item.size() && n_new < m; ++q) {
        while (v < cap && (rows->state[v] & RSK_CONN_LIVE)) ++v;
        if (v == cap) break;
        const uint32_t x = got_item[q], o = got_offer[q];
        const K2 k = item_key(x);
        rows->conn_key[v] = k.first;
        if (by_id) std::memcpy(rows->id + 8ull * v, &k.second, 8);
        rows->src[v] = of.src[o];
        rows->dst[v] = of.dst[o];
        rows->sp[v] = of.sp[o];
        rows->dp[v] = of.dp[o];
        rows->flag[v] = of.flag[o];
        rows->seq[v] = rsk::create_seq(of.ack[o]);
        rows->ack[v] = rsk::create_ack(of.ack[o]);
        if (in->established_ms) in->established_ms[v] = in->now_ms;
        if (in->ka_tries) in->ka_tries[v] = (uint8_t)RSK_KA_NONE;
        rows->state[v] = (uint8_t)(RSK_CONN_LIVE | RSK_CONN_ALIVE | RSK_CONN_NEW);
        uint32_t s = rsk::conn_home(k.first, k.second, slots);  // rsk_conn_index_build's rule, bounded
        for (uint32_t step = 0; step < slots; ++step, s = rsk::conn_next(s, slots)) {
            const uint32_t e = t->index[s];
            if (e == rsk::kConnEmpty) { t->index[s] = v; break; }
            if (e >= cap) break;
            if (h.key(e) == k.first && (!by_id || h.id(e) == k.second)) {
                if (v < e) t->index[s] = v;
                break;
            }
        }
        if (out->new_rows) out->new_rows[n_new] = v;
        if (out->new_first && !list) out->new_first[n_new] = x;
        if (out->new_offer) out->new_offer[n_new] = o;
        if (out->offer_row) out->offer_row[o] = v;
        ++n_new;
        ++v;
    }
    if (out->pick) {
        if (n_new) pick_refresh_host(t, out->pick);
        if (out->pick_counts) {
            out->pick_counts[0] = out->pick[1];
            out->pick_counts[1] = out->pick[0];
        }
    }
    if (!list) {
        uint32_t left = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (out->miss[i] != RSK_RECV_VALID) continue;
            const uint32_t row = rsk::conn_lookup(h, cap, by_id, in->conn_key[i], by_id ? load64(in->id + 8ull * i) : 0ull);
            if (row == RSK_CONN_NONE) { ++left; continue; }
            out->conn[i] = row;
            if (out->hit) out->hit[i] = 1;
            out->miss[i] = RSK_RECV_DROP;
        }
        if (out->n_miss) *out->n_miss = left;
    }
    if (out->n_new) *out->n_new = n_new;
    if (out->n_full) *out->n_full = (uint32_t)got_item.size() - n_new;
    if (out->n_refused) *out->n_refused = keys - (uint32_t)got_item.size();
    return RSK_OK;
}

// ---- conv table (rsk_conv_table): the host twins; the index is the connection table's --------------------
namespace {

constexpr uint32_t kConvFlags = RSK_CONV_BY_DST | RSK_CONV_BY_ID;

struct HostConvTab {
    const rsk_conv_table *t;
    uint32_t entry(uint32_t s) const { return t->index[s]; }
    uint64_t key(uint32_t row) const {
        const uint64_t c = t->conv[row];
        return (t->flags & RSK_CONV_BY_DST) ? ((uint64_t)t->dst[row] << 32) | c : c;
    }
    uint64_t id(uint32_t row) const { return load64(t->id + 8ull * row); }
};

bool conv_tab_ok(const rsk_conv_table *t) {
    return t && !(t->flags & ~kConvFlags) && t->capacity >= 1u && t->capacity <= RSK_CONN_MAX_ROWS;
}
bool conv_tab_lookup_ok(const rsk_conv_table *t) {
    return conv_tab_ok(t) && t->state && t->conv && t->index && (!(t->flags & RSK_CONV_BY_DST) || t->dst) &&
           (!(t->flags & RSK_CONV_BY_ID) || t->id);
}

}  // namespace

extern "C" int rsk_conv_index_build_host(const rsk_conv_table *t, uint32_t *n_dup, int /*nthreads*/) {
    if (!conv_tab_lookup_ok(t)) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(t->index) & 15u) return RSK_EINVAL;
    index_build_host(HostConvTab{t}, t->index, t->state, t->capacity, (t->flags & RSK_CONV_BY_ID) != 0, n_dup);
    return RSK_OK;
}

// The lookups over shards; then one walk in packet order for the counts, the resets' rows and the list.
extern "C" int rsk_conv_resolve_host(const rsk_conv_table *t, uint32_t n, const rsk_conv_resolve_in *in,
                                     const rsk_conv_resolve_out *out, int nthreads) {
    if (!in || !out || !conv_tab_lookup_ok(t)) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONV_BY_ID) != 0, by_dst = (t->flags & RSK_CONV_BY_DST) != 0;
    if (n && (!in->status || !in->conv || !out->conv_row || (by_dst && !in->dst) || (by_id && !in->id))) return RSK_EINVAL;
    if ((in->ctl_kind == nullptr) != (in->ctl_arg == nullptr)) return RSK_EINVAL;
    const bool list = ctl_msgs_any(out->msgs);
    if (list && !out->msgs.n_msg) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    if (out->rst_first) std::memset(out->rst_first, 0xFF, 4ull * t->capacity);
    std::vector<uint8_t> mode(n);  // 0 not looked up, 1 DATA, 2 CONV_RST
    uint8_t *md = mode.data();
    const rsk_conv_resolve_in a = *in;
    uint32_t *rows = out->conv_row;
    const HostConvTab h{t};
    const uint32_t cap = t->capacity;
    for_shards(n, nthreads, [=](uint32_t lo, uint32_t hi) {
        for (uint32_t i = lo; i < hi; ++i) {
            const bool ex = a.status[i] == RSK_RECV_VALID && (!a.cmd || a.cmd[i] == RSK_CMD_DATA) && (!a.hit || a.hit[i]);
            const bool rst = !ex && a.ctl_kind && by_dst && a.ctl_kind[i] == RSK_CTL_CONV_RST;
            uint32_t row = RSK_CONN_NONE;
            if (ex || rst) {
                uint64_t key = ex ? (uint64_t)a.conv[i] : (uint64_t)(uint32_t)a.ctl_arg[i];
                if (by_dst) key |= (uint64_t)a.dst[i] << 32;
                row = rsk::conn_lookup(h, cap, by_id, key, by_id ? load64(a.id + 8ull * i) : 0ull);
            }
            md[i] = ex ? 1 : rst ? 2 : 0;
            rows[i] = row;
        }
    });
    uint32_t n_unk = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t row = rows[i];
        const bool unk = mode[i] == 1 && row == RSK_CONN_NONE;
        if (out->unknown) out->unknown[i] = unk ? (int8_t)RSK_RECV_VALID : (int8_t)RSK_RECV_DROP;
        if (row != RSK_CONN_NONE) {
            if (mode[i] == 1 && t->cur_in) ++t->cur_in[row];
            if (mode[i] == 2 && out->rst_first && out->rst_first[row] == 0xFFFFFFFFu) out->rst_first[row] = i;
        }
        if (unk) {
            if (list) {
                ctl_put_msg(out->msgs, n_unk, RSK_CMD_CONV_RST, in->conv[i], in->id ? in->id + 8ull * i : nullptr, i, 0ull);
                if (out->msgs.pay_len) out->msgs.pay_len[n_unk] = 4;  // encode_uint32 (ConnReset.cpp:34-41)
            }
            ++n_unk;
        }
    }
    if (out->msgs.n_msg) *out->msgs.n_msg = n_unk;
    if (out->n_unknown) *out->n_unknown = n_unk;
    return RSK_OK;
}

extern "C" int rsk_conv_send_host(const rsk_conv_table *t, uint32_t n, const uint32_t *conv_row, const int32_t *sent,
                                  const rsk_conv_send_out *out, int /*nthreads*/) {
    if (!out || !conv_tab_ok(t) || !t->state) return RSK_EINVAL;
    if ((out->conv && !t->conv) || (out->dst && !t->dst) || (out->id && !t->id) || (sent && !t->cur_out)) return RSK_EINVAL;
    if (n && !conv_row) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    uint32_t bad = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t r = conv_row[i];
        const bool ok = r < t->capacity && (t->state[r] & RSK_CONN_LIVE);
        if (out->conv) out->conv[i] = ok ? t->conv[r] : 0u;
        if (out->dst) out->dst[i] = ok ? t->dst[r] : 0u;
        if (out->id) {
            if (ok) std::memcpy(out->id + 8ull * i, t->id + 8ull * r, 8);
            else std::memset(out->id + 8ull * i, 0, 8);
        }
        if (out->ok) out->ok[i] = ok;
        bad += !ok;
        if (ok && sent && sent[i] > 0) ++t->cur_out[r];  // IConn::Send -> afterSend
    }
    if (out->n_bad) *out->n_bad = bad;
    return RSK_OK;
}

extern "C" int rsk_conv_flush_host(const rsk_conv_table *t, const rsk_conv_flush_out *out, int /*nthreads*/) {
    if (!out || !conv_tab_ok(t) || !t->state || !t->alive) return RSK_EINVAL;
    if (!t->cur_in || !t->cur_out || !t->prev_in || !t->prev_out) return RSK_EINVAL;
    if (out->dead_rows && !out->n_dead) return RSK_EINVAL;
    uint32_t n_dead = 0, n_alive = 0;
    for (uint32_t r = 0; r < t->capacity; ++r) {
        if (!(t->state[r] & RSK_CONN_LIVE)) continue;
        if (!t->alive[r]) {  // IGroup::Flush closes it before the flush loop
            if (out->dead_rows) out->dead_rows[n_dead] = r;
            ++n_dead;
            continue;
        }
        // DataStat::Flush (conn/IConn.cpp:70-79)
        const bool alive = t->prev_in[r] != t->cur_in[r] && t->prev_out[r] != t->cur_out[r];
        if (!alive) t->alive[r] = 0;
        t->prev_in[r] = t->cur_in[r];
        t->prev_out[r] = t->cur_out[r];
        n_alive += alive;
    }
    if (out->n_dead) *out->n_dead = n_dead;
    if (out->n_alive) *out->n_alive = n_alive;
    return RSK_OK;
}

extern "C" uint64_t rsk_conv_create_bytes(uint32_t u_max, uint32_t capacity) {
    if (u_max == 0u || u_max > rsk::kCreateMaxU || capacity < 1u || capacity > RSK_CONN_MAX_ROWS) return 0;
    return 4ull * rsk::create_layout(u_max, capacity).words;
}

// One walk over the considered packets in packet order -- a first arrival takes the next vacant row and goes
// into the index at once -- then one over the batch for the packets that now resolve.  The dedup table and
// the list live in `work` as on the device (rsk_conv_create.h).
extern "C" int rsk_conv_create_host(const rsk_conv_table *t, const rsk_conv_rows *rows, uint32_t n,
                                    const rsk_conv_create_in *in, const rsk_conv_create_out *out, int /*nthreads*/) {
    if (!rows || !in || !out || !conv_tab_lookup_ok(t) || !in->work) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONV_BY_ID) != 0, by_dst = (t->flags & RSK_CONV_BY_DST) != 0;
    if (rows->state != t->state || rows->conv != t->conv || (by_dst && rows->dst != t->dst) || (by_id && rows->id != t->id))
        return RSK_EINVAL;
    if (in->u_max == 0u || in->u_max > rsk::kCreateMaxU) return RSK_EINVAL;
    if (n && (!out->conv_row || !out->unknown || !in->conv || (by_dst && !in->dst) || (by_id && !in->id))) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(in->work) & 15u) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    if (out->n_unknown) *out->n_unknown = 0;
    if (out->n_new) *out->n_new = 0;
    if (out->n_full) *out->n_full = 0;
    if (n == 0) return RSK_OK;
    const uint32_t cap = t->capacity, u = in->u_max < n ? in->u_max : n;
    const rsk::CreateLayout l = rsk::create_layout(in->u_max, cap);
    uint32_t *w = static_cast<uint32_t *>(in->work), *dedup = w + l.dedup, *list = w + l.list;
    auto pkt_key = [&](uint32_t i) {
        const uint64_t c = in->conv[i];
        return by_dst ? ((uint64_t)in->dst[i] << 32) | c : c;
    };
    auto pkt_id = [&](uint32_t i) { return by_id ? load64(in->id + 8ull * i) : 0ull; };
    uint32_t m = 0;
    for (uint32_t i = 0; i < n && m < u; ++i)
        if (out->unknown[i] == RSK_RECV_VALID) list[m++] = i;
    const uint32_t dslots = rsk::create_slots(m ? m : 1u);  // as many entries as the considered packets need
    if (m) std::memset(dedup, 0xFF, 4ull * dslots);
    const HostConvTab h{t};
    const uint32_t slots = rsk::conn_slots(cap);
    uint32_t keys = 0, n_new = 0, v = 0;
    for (uint32_t p = 0; p < m; ++p) {
        const uint32_t i = list[p];
        const uint64_t key = pkt_key(i), id = pkt_id(i);
        bool first = false;
        for (uint32_t s = rsk::conn_home(key, id, dslots);; s = rsk::conn_next(s, dslots)) {  // at least half is free
            const uint32_t e = dedup[s];
            if (e == rsk::kConnEmpty) { dedup[s] = p; first = true; break; }
            if (pkt_key(list[e]) == key && pkt_id(list[e]) == id) break;
        }
        if (!first) continue;
        ++keys;
        while (v < cap && (rows->state[v] & RSK_CONN_LIVE)) ++v;
        if (v == cap) continue;
        rows->conv[v] = in->conv[i];
        if (by_dst) rows->dst[v] = in->dst[i];
        if (by_id) std::memcpy(rows->id + 8ull * v, in->id + 8ull * i, 8);
        if (t->cur_in) t->cur_in[v] = 0;
        if (t->cur_out) t->cur_out[v] = 0;
        if (t->prev_in) t->prev_in[v] = 0;
        if (t->prev_out) t->prev_out[v] = 0;
        if (t->alive) t->alive[v] = 1;
        rows->state[v] = RSK_CONN_LIVE;
        // rsk_conv_index_build's rule: a free entry, or the lowest row of the key; an entry that is no row
        // (an index that was never built) ends the walk, as it ends a lookup
        uint32_t s = rsk::conn_home(key, id, slots);
        for (uint32_t step = 0; step < slots; ++step, s = rsk::conn_next(s, slots)) {
            const uint32_t e = t->index[s];
            if (e == rsk::kConnEmpty) { t->index[s] = v; break; }
            if (e >= cap) break;
            if (h.key(e) == key && (!by_id || h.id(e) == id)) {
                if (v < e) t->index[s] = v;
                break;
            }
        }
        if (out->new_rows) out->new_rows[n_new] = v;
        if (out->new_first) out->new_first[n_new] = i;
        ++n_new;
        ++v;
    }
    uint32_t left = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (out->unknown[i] != RSK_RECV_VALID) continue;
        const uint32_t row = rsk::conn_lookup(h, cap, by_id, pkt_key(i), pkt_id(i));
        if (row == RSK_CONN_NONE) { ++left; continue; }
        out->conv_row[i] = row;
        out->unknown[i] = RSK_RECV_DROP;
        if (t->cur_in) ++t->cur_in[row];
    }
    if (out->n_unknown) *out->n_unknown = left;
    if (out->n_new) *out->n_new = n_new;
    if (out->n_full) *out->n_full = keys - n_new;
    return RSK_OK;
}

extern "C" uint64_t rsk_conv_close_bytes(uint32_t capacity) {
    if (capacity < 1u || capacity > RSK_CONN_MAX_ROWS) return 0;
    return ((uint64_t)capacity + 15u) & ~15ull;
}

// The marks (timer form: in `work`, as on the device), the packets behind their row's reset, then the rows in
// order; the index is rebuilt over the rows that stay only when a row closed.
extern "C" int rsk_conv_close_host(const rsk_conv_table *t, const rsk_conv_rows *rows, uint32_t n,
                                   const rsk_conv_close_in *in, const rsk_conv_close_out *out, int /*nthreads*/) {
    if (!rows || !in || !out || !conv_tab_lookup_ok(t)) return RSK_EINVAL;
    const bool by_id = (t->flags & RSK_CONV_BY_ID) != 0, by_dst = (t->flags & RSK_CONV_BY_DST) != 0;
    if (rows->state != t->state || rows->conv != t->conv || (by_dst && rows->dst != t->dst) || (by_id && rows->id != t->id))
        return RSK_EINVAL;
    const bool timer = in->close_rows != nullptr, recv = in->rst_first != nullptr;
    if (timer == recv || (in->flags & ~RSK_CONV_CLOSE_HOLD)) return RSK_EINVAL;
    const bool hold = (in->flags & RSK_CONV_CLOSE_HOLD) != 0;
    if (timer && (!in->n_close || !in->work || n != 0u || hold || in->ctl_kind)) return RSK_EINVAL;
    if (recv && (in->n_close || (n && (!in->ctl_kind || !out->conv_row)))) return RSK_EINVAL;
    if ((out->closed_rows || out->closed_at) && !out->n_closed) return RSK_EINVAL;
    if (reinterpret_cast<uintptr_t>(t->index) & 15u) return RSK_EINVAL;
    if (timer && (reinterpret_cast<uintptr_t>(in->work) & 15u)) return RSK_EINVAL;
    if (n > RSK_MAX_BATCH) return RSK_EINVAL;
    const uint32_t cap = t->capacity;
    uint8_t *mark = timer ? static_cast<uint8_t *>(in->work) : nullptr;
    if (timer) {
        std::memset(mark, 0, (size_t)rsk_conv_close_bytes(cap));
        const uint32_t m = *in->n_close < in->m_max ? *in->n_close : in->m_max;
        for (uint32_t j = 0; j < m; ++j)
            if (in->close_rows[j] < cap) mark[in->close_rows[j]] = 1;
    }
    auto closes = [&](uint32_t r) {
        return (rows->state[r] & RSK_CONN_LIVE) && (timer ? mark[r] != 0 : in->rst_first[r] != 0xFFFFFFFFu);
    };
    uint32_t n_re = 0, n_again = 0, n_closed = 0;
    for (uint32_t i = 0; recv && i < n; ++i) {
        const uint32_t r = out->conv_row[i];
        if (r >= cap || !closes(r) || i <= in->rst_first[r]) continue;
        out->conv_row[i] = RSK_CONN_NONE;
        if (in->ctl_kind[i] == RSK_CTL_CONV_RST) {
            ++n_again;
            continue;
        }
        if (out->unknown) out->unknown[i] = RSK_RECV_VALID;
        ++n_re;
    }
    std::vector<uint32_t> held;
    for (uint32_t r = 0; r < cap; ++r) {
        if (!closes(r)) continue;
        if (out->closed_rows) out->closed_rows[n_closed] = r;
        if (out->closed_at) out->closed_at[n_closed] = timer ? 0xFFFFFFFFu : in->rst_first[r];
        ++n_closed;
        rows->state[r] = (uint8_t)(rows->state[r] & ~RSK_CONN_LIVE);
        if (hold) held.push_back(r);
    }
    if (n_closed) index_build_host(HostConvTab{t}, t->index, t->state, cap, by_id, nullptr);
    for (uint32_t r : held) rows->state[r] |= RSK_CONN_LIVE;  // HOLD: only the index forgets the row
    if (out->n_closed) *out->n_closed = n_closed;
    if (out->n_reopened) *out->n_reopened = n_re;
    if (out->n_rst_again) *out->n_rst_again = n_again;
    if (out->n_unknown) *out->n_unknown += n_re;
    return RSK_OK;
}

// ---- tuple pool ---------------------------------------------------------------------------------------------
namespace {

struct HostPool {
    const rsk_pool *p;
    uint32_t entry(uint32_t s) const { return p->index[s]; }
    uint64_t key(uint32_t row) const { return rsk::tuple_key(p->src[row], p->dst[row]); }
    uint64_t id(uint32_t row) const { return rsk::tuple_ports(p->sp[row], p->dp[row]); }
};

// The LIVE row of a tuple, or RSK_CONN_NONE.  An index that was never built may name a row that is not LIVE.
uint32_t pool_find(const rsk_pool *p, uint64_t key, uint64_t ports) {
    const uint32_t r = rsk::conn_lookup(HostPool{p}, p->capacity, true, key, ports);
    return r < p->capacity && (p->state[r] & RSK_POOL_LIVE) ? r : RSK_CONN_NONE;
}

// The marked rows (settle) or the expired ones (flush, mark == nullptr) leave in row order; the listed ones (the
// settle's purged rows, every row of the flush) go to list.  The index is rebuilt only when a row left.
void pool_leave(const rsk_pool *p, const uint8_t *mark, uint64_t now, uint32_t *list, uint32_t *n_listed) {
    uint32_t left = 0, nl = 0;
    for (uint32_t r = 0; r < p->capacity; ++r) {
        if (!(p->state[r] & RSK_POOL_LIVE)) continue;
        if (mark ? mark[r] == rsk::kPoolStays : p->expiry[r] > now) continue;
        if (!mark || mark[r] == rsk::kPoolPurged) {
            if (list) list[nl] = r;
            ++nl;
        }
        p->state[r] = (uint8_t)(p->state[r] & ~RSK_POOL_LIVE);
        ++left;
    }
    if (left) index_build_host(HostPool{p}, p->index, p->state, p->capacity, true, nullptr);
    if (n_listed) *n_listed = nl;
}

}  // namespace

extern "C" int rsk_pool_index_build_host(const rsk_pool *p, uint32_t *n_dup, int /*nthreads*/) {
    if (!rsk::pool_ok(p, false)) return RSK_EINVAL;
    index_build_host(HostPool{p}, p->index, p->state, p->capacity, true, n_dup);
    return RSK_OK;
}

extern "C" uint64_t rsk_pool_add_bytes(uint32_t u_max, uint32_t capacity) { return rsk_conv_create_bytes(u_max, capacity); }

extern "C" uint64_t rsk_pool_settle_bytes(uint32_t cap_ack, uint32_t cap_sock) {
    if (!rsk::pool_cap_ok(cap_ack) || !rsk::pool_cap_ok(cap_sock)) return 0;
    return rsk::pool_settle_bytes(cap_ack, cap_sock);
}

// One walk over the considered rows in input order: a tuple the pool holds is touched, a new one takes the next
// vacant row and goes into the index at once, so its later arrivals find it there.
extern "C" int rsk_pool_add_host(const rsk_pool *p, uint32_t n, const rsk_pool_add_in *in, const rsk_pool_add_out *out,
                                 int /*nthreads*/) {
    if (!rsk::pool_add_args_ok(p, n, in, out)) return RSK_EINVAL;
    const uint32_t cap = p->capacity, slots = rsk::conn_slots(cap);
    const bool touch = (in->flags & RSK_POOL_TOUCH) != 0;
    const HostPool h{p};
    auto considered = [&](uint32_t i) { return !in->parse_status || in->parse_status[i] == RSK_PARSE_SYN; };
    auto ports_ok = [&](uint32_t i) { return in->sp[i] != 0 && in->dp[i] != 0; };
    uint32_t n_new = 0, n_again = 0, n_zero = 0, taken = 0, v = 0;
    std::map<std::pair<uint64_t, uint64_t>, int> refused;  // the tuples a full pool left without a row
    for (uint32_t i = 0; i < n; ++i) {
        if (!considered(i)) continue;
        if (!ports_ok(i)) { ++n_zero; continue; }
        if (taken == in->u_max) continue;
        ++taken;
        const uint64_t key = rsk::tuple_key(in->src[i], in->dst[i]), ports = rsk::tuple_ports(in->sp[i], in->dp[i]);
        const uint32_t r = pool_find(p, key, ports);
        if (r != RSK_CONN_NONE) {
            ++n_again;
            if (touch) p->expiry[r] = in->expiry;
            continue;
        }
        while (v < cap && (p->state[v] & RSK_POOL_LIVE)) ++v;
        if (v == cap) {
            if (!refused.emplace(std::make_pair(key, ports), 0).second) ++n_again;
            continue;
        }
        p->src[v] = in->src[i];
        p->dst[v] = in->dst[i];
        p->sp[v] = in->sp[i];
        p->dp[v] = in->dp[i];
        if (p->seq) p->seq[v] = in->seq[i];
        if (p->ack) p->ack[v] = in->ack[i];
        p->expiry[v] = in->expiry;
        p->state[v] = RSK_POOL_LIVE;
        // rsk_pool_index_build's rule: a free entry, or the lowest row of the tuple; an entry that is no row (an
        // index that was never built) ends the walk, as it ends a lookup
        uint32_t s = rsk::conn_home(key, ports, slots);
        for (uint32_t step = 0; step < slots; ++step, s = rsk::conn_next(s, slots)) {
            const uint32_t e = p->index[s];
            if (e == rsk::kConnEmpty) { p->index[s] = v; break; }
            if (e >= cap) break;
            if (h.key(e) == key && h.id(e) == ports) {
                if (v < e) p->index[s] = v;
                break;
            }
        }
        if (out->new_rows) out->new_rows[n_new] = v;
        if (out->new_first) out->new_first[n_new] = i;
        ++n_new;
        ++v;
    }
    for (uint32_t i = 0; out->row && i < n; ++i)
        out->row[i] = considered(i) && ports_ok(i)
                          ? pool_find(p, rsk::tuple_key(in->src[i], in->dst[i]), rsk::tuple_ports(in->sp[i], in->dp[i]))
                          : RSK_CONN_NONE;
    if (out->n_new) *out->n_new = n_new;
    if (out->n_again) *out->n_again = n_again;
    if (out->n_full) *out->n_full = (uint32_t)refused.size();
    if (out->n_zero_port) *out->n_zero_port = n_zero;
    return RSK_OK;
}

extern "C" int rsk_pool_offers_host(const rsk_pool *pa, const rsk_pool *ps, const rsk_pool_offers_out *out, int /*nthreads*/) {
    if (!rsk::pool_offers_args_ok(pa, ps, out)) return RSK_EINVAL;
    const HostPool h{pa};
    uint32_t total = 0;
    for (uint32_t r = 0; r < pa->capacity; ++r) {
        if (!(pa->state[r] & RSK_POOL_LIVE)) continue;
        const uint32_t sr = pool_find(ps, h.key(r), h.id(r));
        if (sr == RSK_CONN_NONE) continue;
        const uint32_t o = total++;
        if (o >= out->m_max) continue;
        out->src[o] = pa->src[r];
        out->dst[o] = pa->dst[r];
        out->sp[o] = pa->sp[r];
        out->dp[o] = pa->dp[r];
        out->ack[o] = pa->ack[r];   // the record's ack, never its seq
        out->flag[o] = RSK_TH_ACK;  // the flag the conn sends with, never the handshake's
        if (out->conn_key) out->conn_key[o] = rsk_key_for_tcp(pa->sp[r], pa->dp[r]);
        if (out->offer_ack_row) out->offer_ack_row[o] = r;
        if (out->offer_sock_row) out->offer_sock_row[o] = sr;
    }
    const uint32_t no = total < out->m_max ? total : out->m_max;
    *out->n_offer = no;
    if (out->n_over) *out->n_over = total - no;
    return RSK_OK;
}

extern "C" int rsk_pool_settle_host(const rsk_pool *pa, const rsk_pool *ps, uint32_t n, const rsk_pool_settle_in *in,
                                    const rsk_pool_settle_out *out, int /*nthreads*/) {
    if (!rsk::pool_settle_args_ok(pa, ps, n, in, out)) return RSK_EINVAL;
    uint8_t *mark_a = static_cast<uint8_t *>(in->work), *mark_s = mark_a + rsk::pool_round16(pa->capacity);
    std::memset(mark_a, 0, (size_t)rsk::pool_settle_bytes(pa->capacity, ps->capacity));
    const uint32_t m = in->new_max ? (*in->n_new < in->new_max ? *in->n_new : in->new_max) : 0u;
    for (uint32_t j = 0; j < m; ++j) {  // (a)
        const uint32_t o = in->new_offer[j];
        uint32_t sr = RSK_CONN_NONE;
        if (o < in->m_max) {
            const uint32_t ar = in->offer_ack_row[o];
            sr = in->offer_sock_row[o];
            if (ar < pa->capacity) mark_a[ar] = rsk::kPoolTaken;
            if (sr < ps->capacity) mark_s[sr] = rsk::kPoolTaken;
            else sr = RSK_CONN_NONE;
        }
        if (out->taken_sock_rows) out->taken_sock_rows[j] = sr;
    }
    for (uint32_t i = 0; i < n; ++i) {  // (b)
        if (in->miss[i] != RSK_RECV_VALID) continue;
        const uint64_t key = rsk::tuple_key(in->src[i], in->dst[i]), ports = rsk::tuple_ports(in->sp[i], in->dp[i]);
        const uint32_t ra = pool_find(pa, key, ports), rs = pool_find(ps, key, ports);
        const bool in_a = ra != RSK_CONN_NONE && mark_a[ra] != rsk::kPoolTaken;
        const bool in_s = rs != RSK_CONN_NONE && mark_s[rs] != rsk::kPoolTaken;
        if (in_a == in_s) continue;
        if (in_a) mark_a[ra] = rsk::kPoolPurged;
        else mark_s[rs] = rsk::kPoolPurged;
    }
    pool_leave(pa, mark_a, 0, nullptr, out->n_purged_ack);
    pool_leave(ps, mark_s, 0, out->closed_sock_rows, out->n_closed);
    return RSK_OK;
}

extern "C" int rsk_pool_flush_host(const rsk_pool *p, uint64_t now_ms, const rsk_pool_flush_out *out, int /*nthreads*/) {
    if (!rsk::pool_flush_args_ok(p, out)) return RSK_EINVAL;
    pool_leave(p, nullptr, now_ms, out->dead_rows, out->n_dead);
    return RSK_OK;
}

extern "C" int rsk_stage_capture_slots(uint32_t n, const uint8_t *arena, const uint64_t *cap_off, const uint32_t *cap_len,
                                       uint32_t slot, uint8_t *slots, int nthreads) {
    if (slot < RSK_CAP_SLOT_MIN || (slot & 15u)) return RSK_EINVAL;
    if (n && (!arena || !cap_off || !cap_len || !slots)) return RSK_EINVAL;
    for_shards(n, nthreads, [=](uint32_t lo, uint32_t hi) {
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t k = cap_len[i] < slot ? cap_len[i] : slot;
            uint8_t *d = slots + (uint64_t)slot * i;
            std::memcpy(d, arena + cap_off[i], k);
            std::memset(d + k, 0, slot - k);
        }
    });
    return RSK_OK;
}

extern "C" {

// The 32-B decode slot of one received frame (EncHead::DecodeBuf reads frame[8] = len; the
// hashed byte is frame[8 + len] when that lies inside the frame, RConn.cpp:64-75).
void rsk_stage_decode_header(const uint8_t *frame, int nread, uint8_t *slot) {
    const int k = nread < 0 ? 0 : (nread < 32 ? nread : 32);
    std::memcpy(slot, frame, (size_t)k);
    if (k < 32) std::memset(slot + k, 0, (size_t)(32 - k));
    if (nread > 8) {
        const int at = 8 + frame[8];
        if (at < nread) slot[31] = frame[at];
    }
}

// BuildFilterStr (cap/cap_util.cpp:67-144) with proto "tcp" (cap/RCap.cpp:64)
int rsk_filter_str(const rsk_capture_filter *f, char *buf, size_t buf_len) {
    if (!f || !buf) return -1;
    auto ip = [](uint32_t v) {
        return std::to_string(v & 255u) + "." + std::to_string((v >> 8) & 255u) + "." +
               std::to_string((v >> 16) & 255u) + "." + std::to_string(v >> 24);
    };
    auto ports = [](const rsk_port_list &pl, const char *dir) -> std::string {
        if (pl.n_single == 0 && pl.n_range == 0) return "";
        std::string s = "(";
        for (uint32_t q = 0; q < pl.n_single && q < RSK_FILTER_MAX_PORTS; ++q)
            s += std::string(" or ") + dir + " port " + std::to_string(pl.single[q]);
        for (uint32_t q = 0; q < pl.n_range && q < RSK_FILTER_MAX_PORTS; ++q)
            s += std::string(" or ") + dir + " portrange " + std::to_string(pl.range[q][0]) + "-" +
                 std::to_string(pl.range[q][1]);
        s += " )";
        s.replace(s.find("or"), 2, "");  // the reference removes the first "or"
        return " and " + s;
    };
    std::string out = "tcp";
    if (f->has_src_ip) out += " and  (ip src " + ip(f->src_ip) + ")";
    if (f->has_dst_ip) out += " and  (ip dst " + ip(f->dst_ip) + ")";
    out += ports(f->src_ports, "src");
    out += ports(f->dst_ports, "dst");
    if (f->is_server) {
        std::string s = out;
        for (size_t pos = s.find("dst"); pos != std::string::npos; pos = s.find("dst")) s.replace(pos, 3, "src");
        out = "((tcp[tcpflags] & tcp-syn != 0) and " + s + ") or (" + out + "and (tcp[tcpflags] & (tcp-syn) == 0))";
    }
    if (out.size() + 1 > buf_len) return -1;
    std::memcpy(buf, out.c_str(), out.size() + 1);
    return (int)out.size();
}

uint64_t rsk_key_for_tcp(uint16_t sp, uint16_t dp) {
    return 0x10000000ull | ((uint64_t)dp << 16) | (uint64_t)sp;  // KeyGenerator.cpp:16-25
}
uint64_t rsk_key_for_udp(uint16_t sp, uint16_t dp) {
    return 0x20000000ull | ((uint64_t)dp << 16) | (uint64_t)sp;  // KeyGenerator.cpp:27-36
}

}  // extern "C"
