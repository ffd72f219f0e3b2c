/*
 * transport_packet_echo_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd transport_packet_echo_check;
 * tests/test_transport_packet_echo_host.py).
 *
 * The packet echo's host-only half (csrc/transport_plan.h, header section 14)
 * on the CPU under ASan/UBSan.  On one side the device pipeline's
 * host-compilable parts: the classification and the sort key of
 * tr_packet_keys with its pre-check against the window as it stands,
 * std::stable_sort in place of rocprim's, then one walk of every slot's run
 * (tr_run_head, tr_run_walk) under the echo's rule for one packet,
 * tr_echo_judge, with the descriptor bookkeeping of tr_packet_echo.  On the
 * other side the definition, written here without any of that: the packets
 * one by one in list order through an open, over a window kept as a set of
 * accepted counters, then the accepted ones in list order through a seal.
 * The AEAD is not here: whether a packet's tag verifies is part of the case.
 * Every array is a heap array of exactly its length.
 *   - random lists over few and many slots with preset windows and sends
 *     within 0 .. 4 of the limit, packets of class 6 and 4 mixed in, n == 0;
 *   - every packet on one slot: the list around the window's lower edge,
 *     duplicates inside the run, jumps of top by 1023, 1024 and 2^20, forged
 *     packets between good ones, the counters 0, 2^64 - 2 and 2^64 - 1, each
 *     under every send from 2^64 - 6 to 2^64 - 1;
 *   - the rule alone under the AEAD statuses 0, 1 and 2;
 *   - the argument checks of _echo_packets, which are tr_check_packets's,
 *     against a byte-by-byte reading of the header, over never-dereferenced
 *     pointers.
 *
 * Output: the last line "transport_packet_echo_check: <checks> checks
 * <failures> failures".
 */
#include "../csrc/transport_plan.h"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

using namespace na;

static long g_checks, g_failures;

static void fail(const char *what, const std::string &detail)
{
    if (++g_failures <= 20) fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

typedef unsigned __int128 u128;
static const uint64_t MAXC = ~0ull;

/* a heap array of exactly n items (none: a null pointer) */
template <class T>
struct Heap {
    T *p;
    size_t n;
    explicit Heap(size_t n_) : p(n_ ? (T *)calloc(n_, sizeof(T)) : nullptr), n(n_) {}
    ~Heap() { free(p); }
    Heap(const Heap &) = delete;
    T &operator[](size_t i) { return p[i]; }
};

struct Packet {
    uint32_t slot, len;
    uint64_t counter;
    bool forged;
};

/* a slot as a case gives it: the window as top and the accepted counters of top - 1024 .. top - 1 */
struct Slot {
    bool keyed;
    uint64_t top, send;
    std::set<uint64_t> seen;
};

struct Case {
    std::vector<Slot> slots;
    std::vector<Packet> packets;
};

struct Result {
    std::vector<uint8_t> status;
    std::vector<uint64_t> taken; /* the send counter of an echoed packet, else 0 */
    std::vector<Slot> slots;     /* after the call */
};

/* ---- the definition: an open of the list, then a seal of what it accepted */

static bool fresh(const Slot &s, uint64_t c)
{
    if (c == MAXC) return false;
    if (c >= s.top) return true;
    return s.top - c <= 1024 && !s.seen.count(c);
}

static Result by_definition(const Case &c)
{
    const size_t count = c.packets.size();
    Result r = {std::vector<uint8_t>(count), std::vector<uint64_t>(count), c.slots};
    std::vector<size_t> accepted;
    for (size_t p = 0; p < count; ++p) { /* _open_packets */
        const Packet &k = c.packets[p];
        if (k.slot >= r.slots.size() || !r.slots[k.slot].keyed) r.status[p] = 6;
        else if (k.len < 24 || k.len > 65535) r.status[p] = 4;
        else if (!fresh(r.slots[k.slot], k.counter)) r.status[p] = 5;
        else if (k.forged) r.status[p] = 1;
        else {
            Slot &s = r.slots[k.slot];
            s.seen.insert(k.counter);
            if (k.counter >= s.top) s.top = k.counter + 1;
            accepted.push_back(p);
        }
    }
    for (size_t p : accepted) { /* _seal_packets over the accepted; their slots are keyed and their lengths good */
        Slot &s = r.slots[c.packets[p].slot];
        if (s.send == MAXC) r.status[p] = 5;
        else r.taken[p] = s.send++;
    }
    return r;
}

/* ---- the pipeline of transport.hip */

static void window_of(const Slot &s, TrReplay *w)
{
    memset(w, 0, sizeof *w);
    w->top = s.top;
    for (uint64_t x : s.seen) w->seen[(x / 64) % TR_REPLAY_WORDS] |= 1ull << (x % 64);
}

/* whether the window says what the slot says: top, every counter of top - 1024 .. top - 1, and no bit besides */
static bool window_is(const TrReplay &w, const Slot &s)
{
    if (w.top != s.top) return false;
    uint64_t bits[TR_REPLAY_WORDS] = {0};
    for (uint64_t x : s.seen)
        if (x < s.top && s.top - x <= 1024) bits[(x / 64) % TR_REPLAY_WORDS] |= 1ull << (x % 64);
    return !memcmp(bits, w.seen, sizeof bits);
}

/* tr_packet_echo's functor over the check's arrays: `live` stands for the descriptor (open's or seal's) */
struct Echo {
    uint8_t *status;
    const uint8_t *aead;
    const uint64_t *nonce;
    uint64_t *taken;
    uint8_t *live;
    TrReplay *window;
    uint64_t *send;
    void operator()(uint32_t p) const
    {
        uint64_t c = 0;
        const uint8_t out = tr_echo_judge(window, send, nonce[p], aead[p], &c);
        status[p] = out;
        live[p] = out == 0;
        if (!out) taken[p] = c;
    }
};

static void pipeline(const Case &c, Result &r, std::vector<uint8_t> &live_out)
{
    const uint32_t count = (uint32_t)c.packets.size(), n = (uint32_t)c.slots.size();
    Heap<uint32_t> keys(count), order(count);
    Heap<uint8_t> aead(count), status(count), live(count), keyed(n);
    Heap<uint64_t> nonce(count), taken(count), send(n);
    Heap<TrReplay> replay(n);
    for (uint32_t i = 0; i < n; ++i) {
        keyed[i] = c.slots[i].keyed;
        send[i] = c.slots[i].send;
        window_of(c.slots[i], &replay[i]);
    }
    /* tr_packet_keys, open form */
    for (uint32_t p = 0; p < count; ++p) {
        const Packet &k = c.packets[p];
        const uint8_t cls = tr_packet_class(k.slot, k.len, n, keyed.p);
        keys[p] = tr_packet_key(cls, k.slot, n);
        order[p] = p;
        status[p] = cls;
        aead[p] = TR_STATUS_AEAD_REFUSED;
        nonce[p] = 0xDEADDEADDEADDEADull; /* a refused descriptor's: never looked at */
        if (!cls && tr_replay_check(&replay[k.slot], k.counter)) {
            nonce[p] = k.counter;
            live[p] = 1;
            aead[p] = k.forged ? 1 : 0; /* the AEAD's verdict */
        }
    }
    /* the sort: stable, over the low bits of the keys alone */
    const uint32_t bits = tr_packet_key_bits(n);
    const uint32_t mask = bits == 32 ? ~0u : (1u << bits) - 1;
    {
        std::vector<uint32_t> perm(order.p, order.p + count);
        const uint32_t *kp = keys.p;
        std::stable_sort(perm.begin(), perm.end(), [kp, mask](uint32_t x, uint32_t y) { return (kp[x] & mask) < (kp[y] & mask); });
        Heap<uint32_t> sorted(count);
        for (uint32_t q = 0; q < count; ++q) sorted[q] = keys[perm[q]];
        for (uint32_t q = 0; q < count; ++q) keys[q] = sorted[q], order[q] = perm[q];
    }
    /* tr_packet_echo: one lane per sorted position */
    for (uint32_t q = 0; q < count; ++q) {
        if (!tr_run_head(keys.p, q, n)) continue;
        const uint32_t i = keys[q];
        uint64_t s = send[i];
        tr_run_walk(keys.p, order.p, count, q, Echo{status.p, aead.p, nonce.p, taken.p, live.p, &replay[i], &s});
        send[i] = s;
    }
    r.status.assign(status.p, status.p + count);
    r.taken.assign(taken.p, taken.p + count);
    live_out.assign(live.p, live.p + count);
    r.slots = c.slots;
    for (uint32_t i = 0; i < n; ++i) {
        r.slots[i].send = send[i];
        r.slots[i].top = replay[i].top;
        r.slots[i].seen.clear();
    }
    /* every word of the windows, against the definition's sets */
    const Result want = by_definition(c);
    for (uint32_t i = 0; i < n; ++i) {
        ++g_checks;
        if (!window_is(replay[i], want.slots[i])) fail("window", "slot " + std::to_string(i) + " after the call");
    }
}

static void run_case(const Case &c, const char *what)
{
    const size_t count = c.packets.size();
    const Result want = by_definition(c);
    Result got;
    std::vector<uint8_t> live;
    pipeline(c, got, live);
    ++g_checks;
    for (size_t p = 0; p < count; ++p) {
        if (want.status[p] != got.status[p] || want.taken[p] != got.taken[p] || live[p] != (got.status[p] == 0)) {
            char m[240];
            snprintf(m, sizeof m, "packet %zu of %zu (slot %u, counter %" PRIu64 "): by definition %d counter %" PRIu64
                     ", the pipeline %d counter %" PRIu64 ", descriptor %s", p, count, c.packets[p].slot, c.packets[p].counter,
                     want.status[p], want.taken[p], got.status[p], got.taken[p], live[p] ? "live" : "refused");
            fail(what, m);
            break;
        }
    }
    for (size_t i = 0; i < c.slots.size(); ++i)
        if (want.slots[i].send != got.slots[i].send || want.slots[i].top != got.slots[i].top)
            fail(what, "slot " + std::to_string(i) + ": the send or the window's top after the call");
}

/* ---- the built-in cases */

struct Rng {
    uint64_t x;
    uint64_t next()
    {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return x >> 33;
    }
};

/* a counter at top + d, if it is one */
static bool at(uint64_t top, int64_t d, uint64_t *c)
{
    const __int128 v = (__int128)top + d;
    if (v < 0 || v > (__int128)MAXC) return false;
    *c = (uint64_t)v;
    return true;
}

static Slot slot_with(bool keyed, uint64_t top, uint64_t send, const std::vector<int64_t> &behind)
{
    Slot s = {keyed, top, send, {}};
    uint64_t x;
    for (int64_t d : behind)
        if (d >= 1 && d <= 1024 && at(top, -d, &x)) s.seen.insert(x);
    if (top) s.seen.insert(top - 1); /* top is an accepted counter + 1 */
    return s;
}

static const uint32_t LENS[] = {24, 25, 1424, 65535, 0, 23, 65536, 0xffffffffu};

static void run_random()
{
    for (uint64_t seed = 1; seed <= 60; ++seed) {
        Rng r = {seed * 0x9E3779B97F4A7C15ull};
        Case c;
        const uint32_t n = seed % 10 == 0 ? 0 : seed % 5 == 1 ? 1 : seed % 5 == 2 ? 3 : seed % 5 == 3 ? 67 : 1000;
        const uint64_t bases[] = {0, 5000, 1ull << 40, MAXC - 3000, MAXC - 40};
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t base = bases[r.next() % 5];
            std::vector<int64_t> behind;
            for (int k = 0; k < 40; ++k) behind.push_back(1 + (int64_t)(r.next() % 1024));
            const uint64_t send = r.next() % 3 == 0 ? MAXC - r.next() % 6 : r.next() % 2 ? base : r.next();
            c.slots.push_back(slot_with(r.next() % 8 != 0, base, send, behind));
        }
        const uint32_t count = seed % 7 == 0 ? 1 : 200 + (uint32_t)(r.next() % 900);
        for (uint32_t p = 0; p < count; ++p) {
            Packet k = {};
            const uint64_t pick = r.next() % 16;
            k.slot = pick == 0 ? n : pick == 1 ? 0xffffffffu : pick == 2 ? n + 1 + (uint32_t)(r.next() % 5)
                                                                       : (uint32_t)(r.next() % (n ? n : 1));
            k.len = LENS[r.next() % 10 < 7 ? r.next() % 4 : 4 + r.next() % 4];
            k.forged = r.next() % 9 == 0;
            /* around where the slot's window began: near top, far ahead, far behind, repeats of earlier packets */
            const uint64_t top = k.slot < n ? c.slots[k.slot].top : 0;
            const uint64_t kind = r.next() % 16;
            const int64_t d = kind < 8 ? (int64_t)(r.next() % 60) - 30 : kind < 13 ? (int64_t)(r.next() % 3100) - 1550 : (int64_t)(r.next() % 5000);
            if (kind == 15 && p) k.counter = c.packets[r.next() % p].counter;
            else if (kind == 14) k.counter = r.next() % 2 ? MAXC : MAXC - 1;
            else if (!at(top, d, &k.counter)) k.counter = 0;
            c.packets.push_back(k);
        }
        run_case(c, "random lists");
    }
}

/* every packet on one slot, under every send within 0 .. 4 of the limit and at it, and one far from it */
static void run_one_slot()
{
    const uint64_t tops[] = {0, 1, 1024, 1025, 5 * 1024 + 63, (1ull << 40) + 7, MAXC - 1025, MAXC - 1, MAXC};
    const uint64_t sends[] = {77, MAXC - 5, MAXC - 4, MAXC - 3, MAXC - 2, MAXC - 1, MAXC};
    const int64_t far[] = {1023, 1024, 1 << 20};
    for (uint64_t top : tops)
        for (uint64_t send : sends)
            for (int jump = 0; jump < 3; ++jump) {
                Case c;
                c.slots = {slot_with(true, 9, send, {}), slot_with(false, 0, 0, {}), slot_with(true, 0, 3, {}),
                           slot_with(true, top, send, {1024, 700}), slot_with(true, top, MAXC - 2, {1024, 700})};
                auto add = [&c](uint64_t counter, bool forged) { c.packets.push_back({3, 24 + (uint32_t)(counter % 70), counter, forged}); };
                uint64_t x;
                for (int64_t d = -1026; d <= 2; d += send == 77 ? 1 : 41) /* from below the window's edge to above top */
                    if (at(top, d, &x)) add(x, d % 4 == 0);
                for (int64_t d : {-1025, -1024, -1023, -700, -1, 0, 1, 2}) /* again: the edges, and duplicates inside the run */
                    if (at(top, d, &x)) add(x, false), add(x, false);
                if (at(top, far[jump], &x)) {
                    add(x, true); /* a forged jump moves nothing and takes no counter */
                    add(x, false);
                    add(x, false);
                }
                for (int64_t d = -1026; d <= 2; d += 5) /* what the jump left behind */
                    if (at(top, d, &x)) add(x, false);
                for (uint64_t e : {(uint64_t)0, MAXC - 1, MAXC, MAXC - 1, (uint64_t)0}) add(e, false);
                /* sentinels among them */
                c.packets.insert(c.packets.begin() + 3, Packet{1, 100, 5, false});
                c.packets.insert(c.packets.begin() + std::min<size_t>(30, c.packets.size()), Packet{3, 23, 6, false});
                c.packets.push_back({5, 100, 7, false});
                run_case(c, "one slot");
                /* the same list dealt out to three slots in turn, and so interleaved */
                Case d = c;
                for (size_t p = 0; p < d.packets.size(); ++p)
                    if (d.packets[p].slot == 3) d.packets[p].slot = p % 3 == 0 ? 0 : p % 3 == 1 ? 3 : 4;
                run_case(d, "three slots");
            }
}

/* tr_echo_judge alone: what each AEAD status does to the window and to the send */
static void run_rule()
{
    for (uint64_t send : {(uint64_t)0, MAXC - 4, MAXC - 3, MAXC - 2, MAXC - 1, MAXC})
        for (uint64_t c : {(uint64_t)0, (uint64_t)4999, (uint64_t)5000, (uint64_t)5000 + 1024, (uint64_t)3976, (uint64_t)3975, MAXC - 1, MAXC})
            for (uint8_t s : {(uint8_t)0, (uint8_t)1, (uint8_t)2}) {
                const Slot slot = slot_with(true, 5000, send, {1024});
                TrReplay w, before;
                window_of(slot, &w);
                before = w;
                uint64_t lane = send, taken = 0x5555;
                const bool is_fresh = fresh(slot, c);
                const uint8_t out = tr_echo_judge(&w, &lane, c, s, &taken);
                const uint8_t want = s == 2 || !is_fresh ? 5 : s == 1 ? 1 : send == MAXC ? 5 : 0;
                const bool moved = memcmp(&w, &before, sizeof w) != 0;
                ++g_checks;
                if (out != want || moved != (is_fresh && s == 0) || lane != (want == 0 ? send + 1 : send) ||
                    taken != (want == 0 ? send : 0x5555)) {
                    char m[160];
                    snprintf(m, sizeof m, "send %" PRIu64 " counter %" PRIu64 " AEAD status %d: %d, want %d, send after %" PRIu64, send, c, s,
                             out, want, lane);
                    fail("tr_echo_judge", m);
                }
            }
}

/* ---- the argument rules of _echo_packets, restated byte by byte from the header */

static bool bytes_meet(uint64_t a, u128 a_bytes, uint64_t b, u128 b_bytes)
{
    if (a_bytes > 4096 || b_bytes > 4096) /* too many to count: the ranges as intervals */
        return a_bytes && b_bytes && (u128)a < (u128)b + b_bytes && (u128)b < (u128)a + a_bytes;
    for (u128 x = a; x < (u128)a + a_bytes; ++x)
        if (x >= b && x < (u128)b + b_bytes) return true;
    return false;
}

static const int OK = NOISE_ERROR_NONE, BAD = NOISE_ERROR_INVALID_PARAM, STATE = NOISE_ERROR_INVALID_STATE;

struct Call {
    uint64_t tr;
    uint32_t reserved;
    uint64_t packets;
    uint32_t count;
    uint64_t wire, status;
};

static int rules(const Call &c)
{
    if (!c.tr) return BAD;
    if (c.count == 0) return OK;
    if (!c.reserved) return STATE;
    if (c.count > c.reserved) return BAD;
    if (!c.packets || !c.wire || !c.status) return BAD;
    if (bytes_meet(c.status, c.count, c.packets, (u128)16 * c.count)) return BAD;
    return OK;
}

static const void *ptr(uint64_t v) { return (const void *)(uintptr_t)v; }

static void expect(const Call &c, int want, const char *why)
{
    ++g_checks;
    const int got = tr_check_packets(ptr(c.tr), c.reserved, ptr(c.packets), c.count, ptr(c.wire), ptr(c.status));
    if (got != want || rules(c) != want) {
        char b[300];
        snprintf(b, sizeof b, "%s: got %#x, the rules %#x, want %#x; tr %#" PRIx64 " reserved %u packets %#" PRIx64 " count %u wire %#" PRIx64
                 " status %#" PRIx64, why, got, rules(c), want, c.tr, c.reserved, c.packets, c.count, c.wire, c.status);
        fail("tr_check_packets", b);
    }
}

static void run_rules()
{
    static_assert(sizeof(NoiseAeadPacket) == 16, "the packet of section 13");
    const Call good = {0x10, 256, 0x100000, 3, 0x9000000, 0x200000};
    for (uint32_t reserved : {0u, 1u, 256u, 0x80000000u})
        for (uint32_t count : {0u, 1u, 256u, 257u, 0x80000000u, 0xffffffffu})
            for (int nulls = 0; nulls < 16; ++nulls) {
                Call c = good;
                c.reserved = reserved, c.count = count;
                if (nulls & 1) c.tr = 0;
                if (nulls & 2) c.packets = 0;
                if (nulls & 4) c.wire = 0;
                if (nulls & 8) c.status = 0;
                expect(c, rules(c), "sweep");
            }
    for (uint32_t count : {1u, 3u, 256u}) {
        Call c = good;
        c.count = count;
        c.status = c.packets + 16ull * count;
        expect(c, OK, "touching above");
        c.status -= 1;
        expect(c, BAD, "one byte in from above");
        c.status = c.packets - count;
        expect(c, OK, "touching below");
        c.status += 1;
        expect(c, BAD, "one byte in from below");
        c.status = c.wire; /* the wire is not compared */
        expect(c, OK, "statuses in the wire");
    }
    /* the order, spelled out: each earlier rule wins over every later one */
    Call c = {0, 0, 0, 0, 0, 0};
    expect(c, BAD, "NULL tr before count == 0");
    c.tr = 0x10;
    expect(c, OK, "count == 0, unreserved, before the pointers");
    c.reserved = 8;
    expect(c, OK, "count == 0, reserved");
    c.reserved = 0, c.count = 1;
    expect(c, STATE, "unreserved before the count and the pointers");
    c = good, c.count = 257, c.packets = 0;
    expect(c, BAD, "count > max_packets before the pointers");
    c = good, c.count = 256;
    expect(c, OK, "count == max_packets");
    c = good, c.status = c.packets + 5, c.wire = 0;
    expect(c, BAD, "a NULL pointer before the ranges");
}

int main(int argc, char **argv)
{
    if (argc > 1) fail("argument", argv[1]);
    run_rule();
    run_random();
    run_one_slot();
    run_rules();
    printf("transport_packet_echo_check: %ld checks %ld failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
