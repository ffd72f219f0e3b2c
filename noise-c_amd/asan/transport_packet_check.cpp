/*
 * transport_packet_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd transport_packet_check; tests/test_transport_packet_host.py).
 *
 * Packet transport's host-only half (csrc/transport_plan.h, header section
 * 13) on the CPU under ASan/UBSan: the device pipeline's host-compilable
 * parts — the classification (tr_packet_class), the sort key (tr_packet_key
 * over tr_packet_key_bits bits), std::stable_sort in place of rocprim's, the
 * pre-check against the window as it stands, the run walk (tr_run_head,
 * tr_run_walk) and the commit rule (tr_replay_judge) or the seal's ranks
 * (tr_seal_take) — against plain processing of the packets one by one in list
 * order with tr_replay_check / tr_replay_accept.  The AEAD is not here: whether
 * a packet's tag verifies is part of the case.  Every array is a heap array of
 * exactly its length.
 *   - built in: random lists over few and many slots, every packet on one
 *     slot, duplicates inside a call, jumps of a window or more, the counters
 *     0, 2^64 - 2 and 2^64 - 1, windows preset with the list sitting at
 *     top - 1025 .. top, packets of class 6 and 4 mixed in, n == 0, and seal
 *     ranks with sends that run out;
 *   - from standard input: cases with the caller's expectations (below);
 *   - the argument checks of _reserve_packets and of the two calls against a
 *     byte-by-byte reading of the header, over never-dereferenced pointers.
 *
 * The feed, one directive per line, fields separated by blanks:
 *   open <n> | seal <n>          a new case on a table of n slots, all unkeyed
 *   keyed <slot> ...             these slots are keyed
 *   window <slot> <top> <c> ...  the slot's window: top, and the bits of these counters
 *   send <slot> <value>          the slot's send counter
 *   packet <slot> <len> <counter> <forged 0|1> <status>
 *                                the next packet of the list and the status the
 *                                caller expects for it (seal: counter and forged are 0)
 *   after <slot> <value>         what the caller expects after the call: the
 *                                window's top (open) or the send counter (seal)
 *   run                          run the case
 * The test passes a wrong expectation to see the program compare.
 *
 * Output: the last line "transport_packet_check: <checks> checks <failures>
 * failures".
 */
#include "../csrc/transport_plan.h"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
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
    int expect; /* -1: the caller has none */
};

struct After {
    uint32_t slot;
    uint64_t value;
};

struct Case {
    bool open;
    uint32_t n;
    std::vector<uint32_t> keyed;
    std::vector<std::pair<uint32_t, TrReplay>> windows;
    std::vector<After> sends, after;
    std::vector<Packet> packets;
};

static void window_set(TrReplay *w, uint64_t top, const std::vector<uint64_t> &seen)
{
    memset(w, 0, sizeof *w);
    w->top = top;
    for (uint64_t c : seen) w->seen[(c / 64) % TR_REPLAY_WORDS] |= 1ull << (c % 64);
}

/* the table of a case: state bytes, windows and sends */
struct Table {
    Heap<uint8_t> keyed;
    Heap<TrReplay> replay;
    Heap<uint64_t> send;
    explicit Table(const Case &c) : keyed(c.n), replay(c.n), send(c.n)
    {
        for (uint32_t i : c.keyed) keyed[i] = 1;
        for (const auto &w : c.windows) replay[w.first] = w.second;
        for (const After &s : c.sends) send[s.slot] = s.value;
    }
};

/* ---- the packets one by one, in list order */

static void one_by_one(const Case &c, Table &t, uint8_t *status, uint64_t *counter)
{
    for (size_t p = 0; p < c.packets.size(); ++p) {
        const Packet &k = c.packets[p];
        counter[p] = 0;
        if (k.slot >= c.n || !t.keyed[k.slot]) status[p] = 6;
        else if (k.len < 24 || k.len > 65535) status[p] = 4;
        else if (c.open) {
            TrReplay *w = &t.replay[k.slot];
            if (!tr_replay_check(w, k.counter)) status[p] = 5;
            else if (k.forged) status[p] = 1;
            else {
                tr_replay_accept(w, k.counter);
                status[p] = 0;
            }
        } else if (t.send[k.slot] == MAXC) status[p] = 5;
        else {
            counter[p] = t.send[k.slot]++;
            status[p] = 0;
        }
    }
}

/* ---- the pipeline of transport.hip */

struct Judge {
    uint8_t *status;
    const uint8_t *aead;
    const uint64_t *nonce;
    TrReplay *window;
    void operator()(uint32_t p) const { status[p] = tr_replay_judge(window, nonce[p], aead[p]); }
};

struct Rank {
    uint8_t *status;
    uint64_t *counter, *send;
    void operator()(uint32_t p) const
    {
        uint64_t c;
        if (tr_seal_take(send, &c)) counter[p] = c;
        else status[p] = TR_STATUS_REPLAY;
    }
};

static void pipeline(const Case &c, Table &t, uint8_t *status, uint64_t *counter)
{
    const uint32_t count = (uint32_t)c.packets.size();
    Heap<uint32_t> keys(count), order(count);
    Heap<uint8_t> aead(count);
    Heap<uint64_t> nonce(count);
    /* tr_packet_keys */
    for (uint32_t p = 0; p < count; ++p) {
        const Packet &k = c.packets[p];
        const uint8_t cls = tr_packet_class(k.slot, k.len, c.n, t.keyed.p);
        keys[p] = tr_packet_key(cls, k.slot, c.n);
        order[p] = p;
        status[p] = cls;
        counter[p] = 0;
        aead[p] = TR_STATUS_AEAD_REFUSED;
        nonce[p] = 0xDEADDEADDEADDEADull; /* a refused descriptor's: never looked at */
        if (c.open && !cls && tr_replay_check(&t.replay[k.slot], k.counter)) {
            nonce[p] = k.counter;
            aead[p] = k.forged ? 1 : 0; /* the AEAD's verdict */
        }
    }
    /* the sort: stable, over the low bits of the keys alone */
    const uint32_t bits = tr_packet_key_bits(c.n);
    const uint32_t mask = bits == 32 ? ~0u : (1u << bits) - 1;
    {
        std::vector<uint32_t> perm(order.p, order.p + count);
        const uint32_t *kp = keys.p;
        std::stable_sort(perm.begin(), perm.end(), [kp, mask](uint32_t x, uint32_t y) { return (kp[x] & mask) < (kp[y] & mask); });
        Heap<uint32_t> sorted(count);
        for (uint32_t q = 0; q < count; ++q) sorted[q] = keys[perm[q]];
        for (uint32_t q = 0; q < count; ++q) keys[q] = sorted[q], order[q] = perm[q];
    }
    /* tr_packet_seal / tr_packet_commit: one lane per sorted position */
    for (uint32_t q = 0; q < count; ++q) {
        if (!tr_run_head(keys.p, q, c.n)) continue;
        const uint32_t i = keys[q];
        if (c.open)
            tr_run_walk(keys.p, order.p, count, q, Judge{status, aead.p, nonce.p, &t.replay[i]});
        else {
            uint64_t send = t.send[i];
            tr_run_walk(keys.p, order.p, count, q, Rank{status, counter, &send});
            t.send[i] = send;
        }
    }
}

static void run_case(const Case &c, const char *what)
{
    const size_t count = c.packets.size();
    Table a(c), b(c);
    Heap<uint8_t> sa(count), sb(count);
    Heap<uint64_t> ca(count), cb(count);
    one_by_one(c, a, sa.p, ca.p);
    pipeline(c, b, sb.p, cb.p);
    ++g_checks;
    for (size_t p = 0; p < count; ++p) {
        if (sa[p] != sb[p] || ca[p] != cb[p]) {
            char m[200];
            snprintf(m, sizeof m, "%s packet %zu of %zu (slot %u): one by one %d counter %" PRIu64 ", the pipeline %d counter %" PRIu64,
                     c.open ? "open" : "seal", p, count, c.packets[p].slot, sa[p], ca[p], sb[p], cb[p]);
            fail(what, m);
            break;
        }
    }
    if (c.n && (memcmp(a.replay.p, b.replay.p, c.n * sizeof(TrReplay)) || memcmp(a.send.p, b.send.p, c.n * 8)))
        fail(what, "the windows or the sends after the call");
    for (size_t p = 0; p < count; ++p) {
        if (c.packets[p].expect < 0) continue;
        ++g_checks;
        if (c.packets[p].expect != sb[p])
            fail("expect", "packet " + std::to_string(p) + ": status " + std::to_string(sb[p]) + ", expected " +
                               std::to_string(c.packets[p].expect));
    }
    for (const After &e : c.after) {
        ++g_checks;
        const uint64_t got = e.slot < c.n ? (c.open ? b.replay[e.slot].top : b.send[e.slot]) : 0;
        if (e.slot >= c.n || got != e.value)
            fail("expect", "after, slot " + std::to_string(e.slot) + ": " + std::to_string(got) + ", expected " + std::to_string(e.value));
    }
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

static const uint32_t LENS[] = {24, 25, 1424, 65535, 0, 23, 65536, 0xffffffffu};

static void run_random()
{
    for (uint64_t seed = 1; seed <= 60; ++seed) {
        Rng r = {seed * 0x9E3779B97F4A7C15ull};
        Case c = {};
        c.open = seed % 3 != 0;
        c.n = seed % 10 == 0 ? 0 : seed % 5 == 1 ? 1 : seed % 5 == 2 ? 3 : seed % 5 == 3 ? 67 : 1000;
        for (uint32_t i = 0; i < c.n; ++i)
            if (r.next() % 8) c.keyed.push_back(i);
        const uint64_t bases[] = {0, 5000, 1ull << 40, MAXC - 3000, MAXC - 40};
        for (uint32_t i : c.keyed) {
            const uint64_t base = bases[r.next() % 5];
            if (c.open && base) {
                TrReplay w;
                std::vector<uint64_t> seen;
                for (int k = 0; k < 40; ++k) seen.push_back(base - 1 - r.next() % 1024);
                seen.push_back(base - 1);
                window_set(&w, base, seen);
                c.windows.push_back({i, w});
            } else if (!c.open)
                c.sends.push_back({i, r.next() % 4 == 0 ? MAXC - r.next() % 6 : base});
        }
        const uint32_t count = seed % 7 == 0 ? 1 : 200 + (uint32_t)(r.next() % 900);
        for (uint32_t p = 0; p < count; ++p) {
            Packet k = {};
            const uint64_t pick = r.next() % 16;
            k.slot = pick == 0 ? c.n : pick == 1 ? 0xffffffffu : pick == 2 ? c.n + 1 + (uint32_t)(r.next() % 5)
                                                                           : (uint32_t)(r.next() % (c.n ? c.n : 1));
            k.len = LENS[r.next() % 10 < 7 ? r.next() % 4 : 4 + r.next() % 4];
            k.forged = r.next() % 9 == 0;
            k.expect = -1;
            /* around where the slot's window began: near top, far ahead, far behind, repeats of earlier packets */
            uint64_t top = 0;
            for (const auto &w : c.windows)
                if (w.first == k.slot) top = w.second.top;
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

/* every packet on one slot: the list sits at the window's lower edge, with duplicates and a jump of a window or more */
static void run_one_slot()
{
    const uint64_t tops[] = {0, 1, 1024, 1025, 5 * 1024, 5 * 1024 + 63, (1ull << 40) + 7, MAXC - 1025, MAXC - 1, MAXC};
    for (uint64_t top : tops)
        for (int jump = 0; jump < 3; ++jump)
            for (int forged_first = 0; forged_first < 2; ++forged_first) {
                Case c = {};
                c.open = true;
                c.n = 5;
                c.keyed = {0, 3, 4};
                TrReplay w;
                std::vector<uint64_t> seen;
                if (top) seen.push_back(top - 1);
                if (top > 1024) seen.push_back(top - 1024);
                if (top > 700) seen.push_back(top - 700);
                window_set(&w, top, seen);
                c.windows.push_back({3, w});
                auto add = [&c](uint64_t counter, bool forged) { c.packets.push_back({3, 24 + (uint32_t)(counter % 70), counter, forged, -1}); };
                uint64_t x;
                for (int64_t d = -1026; d <= 2; ++d) /* top - 1026 .. top + 2, every one of them */
                    if (at(top, d, &x)) add(x, forged_first && d % 2);
                for (int64_t d : {-1025, -1024, -1023, -700, -1, 0, 1}) /* again: duplicates inside the call */
                    if (at(top, d, &x)) add(x, false);
                const int64_t far[] = {1023, 1024, 1 << 20};
                if (at(top, far[jump], &x)) {
                    add(x, true); /* a forged jump moves nothing */
                    add(x, false);
                    add(x, false);
                }
                for (int64_t d = -1026; d <= 2; d += 5) /* what the jump left behind */
                    if (at(top, d, &x)) add(x, false);
                for (uint64_t e : {(uint64_t)0, MAXC - 1, MAXC, MAXC - 1, (uint64_t)0}) add(e, false);
                /* sentinels among them */
                c.packets.insert(c.packets.begin() + 7, Packet{1, 100, 5, false, -1});
                c.packets.insert(c.packets.begin() + std::min<size_t>(300, c.packets.size()), Packet{3, 23, 6, false, -1});
                c.packets.push_back({5, 100, 7, false, -1});
                run_case(c, "one slot");
                /* the same list dealt out to three slots in turn, and interleaved with itself */
                Case d = c;
                for (size_t p = 0; p < d.packets.size(); ++p)
                    if (d.packets[p].slot == 3) d.packets[p].slot = p % 3 == 0 ? 0 : p % 3 == 1 ? 3 : 4;
                d.windows.push_back({0, w});
                run_case(d, "three slots");
            }
}

static void run_seal_ranks()
{
    for (uint64_t send : {(uint64_t)0, (uint64_t)77, MAXC - 200, MAXC - 3, MAXC - 2, MAXC - 1, MAXC})
        for (uint32_t count : {1u, 2u, 3u, 200u}) {
            Case c = {};
            c.n = 4;
            c.keyed = {0, 2, 3};
            c.sends = {{0, send}, {2, 9}, {3, MAXC - 1}};
            for (uint32_t p = 0; p < count; ++p) {
                c.packets.push_back({0, 24 + p, 0, false, -1});
                if (p % 3 == 0) c.packets.push_back({2, 40, 0, false, -1});
                if (p % 4 == 1) c.packets.push_back({p % 8 == 1 ? 1u : 4u, 40, 0, false, -1}); /* unkeyed, out of range: they take no counter */
                if (p % 5 == 2) c.packets.push_back({0, p % 10 == 2 ? 23u : 65536u, 0, false, -1});
                if (p % 50 == 3) c.packets.push_back({3, 24, 0, false, -1});
            }
            run_case(c, "seal ranks");
        }
}

static void run_key_bits()
{
    for (uint32_t n : {0u, 1u, 2u, 3u, 4u, 67u, 255u, 256u, 65535u, 65536u, 0x7fffffffu, 0x80000000u, 0xffffffffu}) {
        const uint32_t bits = tr_packet_key_bits(n);
        ++g_checks;
        uint32_t want = 1;
        while (want < 32 && ((uint64_t)1 << want) <= n) ++want;
        if (bits != want || bits < 1 || bits > 32 || (bits < 32 && (n >> bits))) fail("tr_packet_key_bits", std::to_string(n));
    }
}

/* ---- the argument rules, restated byte by byte from the header */

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
    const Call good = {0x10, 1000, 0x100000, 3, 0x9000000, 0x200000};
    for (uint32_t reserved : {0u, 1u, 200u, 0x80000000u})
        for (uint32_t count : {0u, 1u, 200u, 201u, 0x80000000u, 0xffffffffu})
            for (int nulls = 0; nulls < 16; ++nulls) {
                Call c = good;
                c.reserved = reserved, c.count = count;
                if (nulls & 1) c.tr = 0;
                if (nulls & 2) c.packets = 0;
                if (nulls & 4) c.wire = 0;
                if (nulls & 8) c.status = 0;
                expect(c, rules(c), "sweep");
            }
    /* the statuses walk across the list */
    for (uint32_t count : {1u, 2u, 5u})
        for (uint64_t status = 0x1000 - 20; status <= 0x1000 + 100; ++status) {
            Call c = good;
            c.count = count, c.packets = 0x1000, c.status = status;
            expect(c, rules(c), "sweep of the statuses");
        }
    for (uint32_t count : {1u, 3u, 200u}) {
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
    c = good, c.reserved = 0;
    expect(c, STATE, "unreserved");
    c = good, c.count = 1001, c.packets = 0;
    expect(c, BAD, "count > max_packets");
    c = good, c.count = 1000;
    expect(c, OK, "count == max_packets");
    c = good, c.reserved = 0x80000000u, c.count = 0x80000000u, c.packets = 0x1000, c.status = 0x1000 + 16ull * 0x80000000u;
    expect(c, OK, "2^31 packets packed");
    c.status -= 1;
    expect(c, BAD, "2^31 packets, one byte in");
    c = good, c.count = 1, c.packets = MAXC - 15, c.status = MAXC - 16;
    expect(c, OK, "a list at the top of memory");
    c.status = MAXC;
    expect(c, BAD, "the status in it");

    /* _reserve_packets */
    for (uint64_t tr : {(uint64_t)0, (uint64_t)0x10})
        for (uint32_t max_packets : {0u, 1u, 200u, 0x80000000u, 0x80000001u, 0xffffffffu})
            for (uint32_t reserved : {0u, 1u, 200u}) {
                ++g_checks;
                int want = OK;
                if (!tr) want = BAD;
                else if (max_packets == 0 || max_packets > 2147483648u) want = BAD;
                else if (reserved) want = STATE;
                if (tr_check_reserve_packets(ptr(tr), max_packets, reserved) != want)
                    fail("tr_check_reserve_packets", std::to_string(tr) + " " + std::to_string(max_packets) + " " + std::to_string(reserved));
            }
}

/* ---- the feed */

static bool run_feed()
{
    Case c = {};
    bool have = false;
    char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string word;
        if (!(in >> word)) continue;
        if (word == "open" || word == "seal") {
            c = Case();
            c.open = word == "open";
            have = bool(in >> c.n);
        } else if (!have) {
            return false;
        } else if (word == "keyed") {
            uint32_t i;
            while (in >> i) {
                if (i >= c.n) return false;
                c.keyed.push_back(i);
            }
        } else if (word == "window") {
            uint32_t i;
            uint64_t top, x;
            if (!(in >> i >> top) || i >= c.n) return false;
            std::vector<uint64_t> seen;
            while (in >> x) seen.push_back(x);
            TrReplay w;
            window_set(&w, top, seen);
            c.windows.push_back({i, w});
        } else if (word == "send" || word == "after") {
            After a;
            if (!(in >> a.slot >> a.value) || (word == "send" && a.slot >= c.n)) return false;
            (word == "send" ? c.sends : c.after).push_back(a);
        } else if (word == "packet") {
            Packet k;
            int forged;
            if (!(in >> k.slot >> k.len >> k.counter >> forged >> k.expect)) return false;
            k.forged = forged != 0;
            c.packets.push_back(k);
        } else if (word == "run") {
            run_case(c, "feed");
            have = false;
        } else
            return false;
    }
    return !have;
}

int main(int argc, char **argv)
{
    if (argc > 1) fail("argument", argv[1]);
    run_key_bits();
    run_random();
    run_one_slot();
    run_seal_ranks();
    run_rules();
    if (!run_feed()) fail("feed", "a line it cannot read, or a case without its run");
    printf("transport_packet_check: %ld checks %ld failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
