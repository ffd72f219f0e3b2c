/*
 * transport_datagram_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd transport_datagram_check; tests/test_transport_datagram_host.py).
 *
 * Datagram transport's host-only half (csrc/transport_plan.h, header section
 * 11) on the CPU under ASan/UBSan:
 *   - the anti-replay window, tr_replay_check and tr_replay_accept as the
 *     kernels run them, against a set of the counters accepted so far, on
 *     sequences that sit at top - 1025, - 1024, - 1023, - 1, top, + 1, + 1023,
 *     + 1024, + 1025 and + 2^40, at the bit positions 63, 64 and 1023, and at
 *     the counters 0, 2^64 - 2 and 2^64 - 1; after every step each bit of the
 *     window is compared with the set;
 *   - tr_walk with 24 as its smallest L, on heap buffers of exactly their
 *     length, against a restatement, and with its default of 16 beside it;
 *   - the argument checks of _seal_datagrams and _open_datagrams against a
 *     byte-by-byte reading of the header, in the stated order, over
 *     never-dereferenced pointers.
 *
 * An argument "expect <accepted> <counter> <0|1>" adds one expectation of the
 * caller's: after counter <accepted> alone was accepted by an empty window,
 * tr_replay_check of <counter> must say fresh (1) or not (0).  The test passes
 * a wrong one to see the program compare.
 *
 * Output: the last line "transport_datagram_check: <checks> checks <failures>
 * failures".
 */
#include "../csrc/transport_plan.h"

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

/* ---- the window against a set of accepted counters */

struct SetModel {
    std::set<uint64_t> seen;
    uint64_t top() const { return seen.empty() ? 0 : *seen.rbegin() + 1; }
    bool fresh(uint64_t c) const
    {
        if (c == MAXC) return false;
        if (seen.count(c)) return false;
        return c >= top() || top() - c <= 1024;
    }
};

struct Pair {
    TrReplay *w; /* on the heap, exactly its 136 bytes */
    SetModel m;
    Pair()
    {
        w = (TrReplay *)malloc(sizeof(TrReplay));
        memset(w, 0, sizeof(TrReplay));
    }
    ~Pair() { free(w); }
    Pair(const Pair &) = delete;

    /* one frame: check, and accept when fresh; then every bit of the window against the set */
    void step(uint64_t c, const char *what)
    {
        const TrReplay before = *w;
        const bool got = tr_replay_check(w, c), want = m.fresh(c);
        ++g_checks;
        if (memcmp(&before, w, sizeof before)) fail(what, "check wrote the window");
        if (got != want) {
            char b[120];
            snprintf(b, sizeof b, "top %" PRIu64 " counter %" PRIu64 ": fresh %d, the set says %d", w->top, c, (int)got, (int)want);
            fail(what, b);
            return;
        }
        if (!got) return;
        tr_replay_accept(w, c);
        m.seen.insert(c);
        ++g_checks;
        if (w->top != m.top()) fail(what, "top after " + std::to_string(c));
        const uint64_t lo = w->top > 1024 ? w->top - 1024 : 0;
        for (uint64_t x = lo; x < w->top; ++x) {
            const bool bit = (w->seen[(x % 1024) / 64] >> (x % 64)) & 1;
            if (bit != (m.seen.count(x) != 0)) {
                fail(what, "bit of " + std::to_string(x) + " after " + std::to_string(c));
                break;
            }
        }
        for (uint64_t x = w->top; x < 1024; ++x) /* nothing accepted up here yet */
            if ((w->seen[x / 64] >> (x % 64)) & 1) {
                fail(what, "a bit above top after " + std::to_string(c));
                break;
            }
    }
};

static const int64_t EDGES[] = {-1025, -1024, -1023, -1, 0, 1, 1023, 1024, 1025, (int64_t)1 << 40};

/* top + d as a counter, if it is one */
static bool at(uint64_t top, int64_t d, uint64_t *c)
{
    const __int128 v = (__int128)top + d;
    if (v < 0 || v > (__int128)MAXC) return false;
    *c = (uint64_t)v;
    return true;
}

static void run_window()
{
    static_assert(sizeof(TrReplay) == 136 && TR_REPLAY_BITS == 1024 && TR_REPLAY_WORDS == 16, "the layout of section 11");
    const uint64_t tops[] = {0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2048 + 63, 2048 + 64, 2048 + 65,
                             5000, (1ull << 40), (1ull << 40) + 1023, (1ull << 40) + 1024, MAXC - 1026, MAXC - 1025,
                             MAXC - 1024, MAXC - 2, MAXC - 1, MAXC};
    for (uint64_t top : tops)
        for (int64_t d1 : EDGES)
            for (int64_t d2 : EDGES) {
                Pair p;
                if (top) p.step(top - 1, "window edges"); /* top is `top` now; MAXC: 2^64 - 2 was accepted */
                if (top > 1024) p.step(top - 1024, "window edges");
                uint64_t c1, c2;
                if (at(top, d1, &c1)) p.step(c1, "window edges");
                if (at(top, d2, &c2)) p.step(c2, "window edges");
                if (at(top, d1, &c1)) p.step(c1, "window edges"); /* again: a replay, or too old by now */
                /* every edge of where top is now, twice */
                const uint64_t now = p.w->top;
                for (int twice = 0; twice < 2; ++twice)
                    for (int64_t d : EDGES) {
                        uint64_t c;
                        if (d <= 1 && at(now, d, &c)) p.step(c, "window edges after");
                    }
            }
    /* the counters at the ends */
    {
        Pair p;
        for (uint64_t c : {(uint64_t)0, (uint64_t)0, MAXC, MAXC - 1, MAXC, MAXC - 1, (uint64_t)0, MAXC - 2, MAXC - 1025, MAXC - 1026})
            p.step(c, "ends");
        if (p.w->top != MAXC) fail("ends", "top is not 2^64 - 1");
    }
    /* the bit positions 63, 64 and 1023, at the bottom, the middle and the top of a window */
    for (uint64_t lap : {(uint64_t)0, (uint64_t)1024, (uint64_t)1024 * 77, (MAXC - 1) / 1024 * 1024 - 1024})
        for (uint64_t pos : {(uint64_t)63, (uint64_t)64, (uint64_t)1023, (uint64_t)0}) {
            Pair p;
            const uint64_t c = lap + pos;
            p.step(c, "bit positions");
            p.step(c, "bit positions");
            for (uint64_t d : {(uint64_t)1, (uint64_t)63, (uint64_t)64, (uint64_t)1022, (uint64_t)1023}) {
                p.step(c + d, "bit positions");
                p.step(c, "bit positions");
                if (c >= d) p.step(c - d, "bit positions");
            }
            p.step(c + 1024, "bit positions"); /* c's own bit, a lap on */
            p.step(c, "bit positions");
            p.step(c + 1, "bit positions");
            p.step(c + 2048 + 1, "bit positions");
        }
    /* walks around top: steps within a window and a half either way, duplicates among them */
    for (uint64_t seed = 1; seed <= 12; ++seed) {
        Pair p;
        uint64_t x = seed * 0x9E3779B97F4A7C15ull;
        const uint64_t start = seed % 3 == 0 ? MAXC - 3000 : seed % 3 == 1 ? 0 : (1ull << 33) - 700;
        if (start) p.step(start, "walk");
        uint64_t last = start;
        for (int k = 0; k < 1500; ++k) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            const uint64_t r = x >> 33;
            uint64_t c;
            const int kind = (int)(r % 16);
            const int64_t d = kind < 8 ? (int64_t)(r / 16 % 40) - 30 : kind < 14 ? (int64_t)(r / 16 % 3100) - 1550 : 0;
            if (kind == 15) c = last;
            else if (!at(p.w->top, d, &c)) continue;
            p.step(c, "walk");
            last = c;
        }
    }
}

/* ---- the walk with 24 as its smallest L */

struct Frame {
    uint64_t k, body;
    uint32_t L;
};

struct Collect {
    std::vector<Frame> *out;
    void operator()(uint64_t k, uint64_t body, uint32_t L) const { out->push_back({k, body, L}); }
};

static std::string frame(uint32_t L, uint8_t fill)
{
    std::string s;
    s.push_back((char)(L >> 8));
    s.push_back((char)(L & 0xff));
    s.append(L, (char)fill);
    return s;
}

static void walk_case(const char *name, const std::string &stream, uint64_t nonce, uint64_t budget, uint32_t min_len)
{
    /* the restatement */
    std::vector<Frame> want;
    uint64_t off = 0;
    int stop = NOISE_ERROR_NONE;
    while (off + 2 <= stream.size()) {
        const uint32_t L = ((uint32_t)(uint8_t)stream[off] << 8) | (uint8_t)stream[off + 1];
        if (off + 2 + L > stream.size()) break;
        if (L < min_len) {
            stop = NOISE_ERROR_INVALID_LENGTH;
            break;
        }
        if (nonce + want.size() == MAXC) {
            stop = NOISE_ERROR_INVALID_NONCE;
            break;
        }
        if (want.size() == budget) break;
        want.push_back({want.size(), off + 2, L});
        off += 2 + L;
    }
    uint8_t *p = (uint8_t *)malloc(stream.size() ? stream.size() : 1); /* exactly the stream: a read past it is ASan's */
    if (stream.empty()) {
        free(p);
        p = nullptr;
    } else
        memcpy(p, stream.data(), stream.size());
    std::vector<Frame> got;
    const TrWalk w = min_len == TR_MAC_LEN ? tr_walk(p, stream.size(), nonce, budget, Collect{&got})
                                           : tr_walk(p, stream.size(), nonce, budget, Collect{&got}, min_len);
    ++g_checks;
    bool same = w.frames == want.size() && w.consumed == off && w.stop == stop && got.size() == want.size();
    for (size_t k = 0; same && k < want.size(); ++k)
        same = got[k].k == want[k].k && got[k].body == want[k].body && got[k].L == want[k].L;
    if (!same) fail("tr_walk", std::string(name) + " min " + std::to_string(min_len));
    if (p && memcmp(p, stream.data(), stream.size())) fail("tr_walk", std::string(name) + ": wrote the stream");
    free(p);
}

static void run_walk()
{
    const std::string five = frame(24, 1) + frame(25, 2) + frame(24 + 1400, 3) + frame(40, 4) + frame(24, 5);
    for (uint32_t min_len : {TR_DATAGRAM_MIN, TR_MAC_LEN}) {
        walk_case("empty", "", 0, TR_NO_BUDGET, min_len);
        walk_case("one byte", std::string(1, '\0'), 0, TR_NO_BUDGET, min_len);
        walk_case("header only", std::string("\x00\x18", 2), 0, TR_NO_BUDGET, min_len);
        for (uint32_t L : {0u, 15u, 16u, 17u, 23u, 24u, 25u, 65535u}) {
            walk_case("one frame", frame(L, 7), 0, TR_NO_BUDGET, min_len);
            walk_case("one frame short by one", frame(L, 7).substr(0, 1 + L), 0, TR_NO_BUDGET, min_len);
            walk_case("after two", frame(24, 1) + frame(100, 2) + frame(L, 7) + frame(24, 3), 9, TR_NO_BUDGET, min_len);
            walk_case("at the budget's end", frame(24, 1) + frame(24, 2) + frame(L, 7), 0, 2, min_len);
        }
        walk_case("trailing byte", frame(24, 1) + std::string(1, '\0'), 0, TR_NO_BUDGET, min_len);
        for (uint64_t nonce : {MAXC, MAXC - 1, MAXC - 3, MAXC - 5, MAXC - 6})
            walk_case("the nonce runs out", five, nonce, TR_NO_BUDGET, min_len);
        walk_case("a runt before the nonce", frame(24, 1) + frame(23, 2), MAXC - 1, TR_NO_BUDGET, min_len);
        for (uint64_t budget : {(uint64_t)0, (uint64_t)1, (uint64_t)3, (uint64_t)5, (uint64_t)6})
            walk_case("budget", five, 0, budget, min_len);
    }
    /* a frame of 16 .. 23 bytes is a frame to the stream calls and a runt to the datagram calls */
    for (uint32_t L = 16; L < 24; ++L) {
        const std::string s = frame(L, 9);
        uint8_t *p = (uint8_t *)malloc(s.size());
        memcpy(p, s.data(), s.size());
        const TrWalk a = tr_walk(p, s.size(), 0, TR_NO_BUDGET), b = tr_walk(p, s.size(), 0, TR_NO_BUDGET, TrNoEmit(), TR_DATAGRAM_MIN);
        free(p);
        ++g_checks;
        if (a.frames != 1 || a.stop != NOISE_ERROR_NONE || b.frames != 0 || b.consumed != 0 || b.stop != NOISE_ERROR_INVALID_LENGTH)
            fail("tr_walk", "the default smallest L at " + std::to_string(L));
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

static const int OK = NOISE_ERROR_NONE, BAD = NOISE_ERROR_INVALID_PARAM;

struct Call {
    uint64_t tr;
    uint32_t n, object_max;
    uint64_t slots;
    uint32_t m, max_frames;
    uint64_t wire, off, len, result, frame_status;
};

static int rules(const Call &c, bool open)
{
    if (!c.tr) return BAD;
    if (c.m == 0) return OK;
    if (c.m > c.n) return BAD;
    if (!c.wire || !c.off || !c.len || !c.result) return BAD;
    if (open && !c.frame_status) return BAD;
    if (c.max_frames > c.object_max) return BAD;
    const u128 rb = (u128)(open ? 24 : 16) * c.m;
    if (bytes_meet(c.result, rb, c.off, (u128)8 * c.m) || bytes_meet(c.result, rb, c.len, (u128)4 * c.m)) return BAD;
    if (c.slots && bytes_meet(c.result, rb, c.slots, (u128)4 * c.m)) return BAD;
    if (open) {
        const u128 cap = c.max_frames ? c.max_frames : c.object_max;
        if (bytes_meet(c.frame_status, cap, c.off, (u128)8 * c.m) || bytes_meet(c.frame_status, cap, c.len, (u128)4 * c.m) ||
            bytes_meet(c.frame_status, cap, c.result, rb))
            return BAD;
        if (c.slots && bytes_meet(c.frame_status, cap, c.slots, (u128)4 * c.m)) return BAD;
    }
    return OK;
}

static const void *ptr(uint64_t v) { return (const void *)(uintptr_t)v; }

static int checked(const Call &c, bool open)
{
    return tr_check_datagrams(ptr(c.tr), c.n, c.object_max, ptr(c.slots), c.m, c.max_frames, ptr(c.wire), ptr(c.off), ptr(c.len),
                              ptr(c.result), open ? sizeof(NoiseAeadDatagramResult) : sizeof(NoiseAeadTransportResult), open,
                              ptr(c.frame_status));
}

static void expect(const Call &c, bool open, int want, const char *why)
{
    ++g_checks;
    const int got = checked(c, open);
    if (got != want || rules(c, open) != want) {
        char b[400];
        snprintf(b, sizeof b, "%s (%s): got %#x, the rules %#x, want %#x; tr %#" PRIx64 " n %u object max %u slots %#" PRIx64
                 " m %u max %u wire %#" PRIx64 " off %#" PRIx64 " len %#" PRIx64 " result %#" PRIx64 " status %#" PRIx64,
                 why, open ? "open" : "seal", got, rules(c, open), want, c.tr, c.n, c.object_max, c.slots, c.m, c.max_frames,
                 c.wire, c.off, c.len, c.result, c.frame_status);
        fail("tr_check_datagrams", b);
    }
}

static void same(const Call &c, bool open) { expect(c, open, rules(c, open), "sweep"); }

static void run_rules()
{
    static_assert(sizeof(NoiseAeadDatagramResult) == 24 && sizeof(NoiseAeadTransportResult) == 16, "the results of section 11");
    const Call good = {0x10, 1000, 64, 0x100000, 3, 0, 0x9000000, 0x200000, 0x300000, 0x400000, 0x500000};
    for (int open = 0; open < 2; ++open) {
        /* NULLs, m against n, the cap against the object's */
        for (uint32_t n : {0u, 1u, 67u, 0xffffffffu})
            for (uint32_t m : {0u, 1u, 67u, 68u, 0xffffffffu})
                for (uint32_t object_max : {1u, 64u, 0x80000000u})
                    for (uint32_t mf : {0u, 1u, 64u, 65u, 0xffffffffu})
                        for (int nulls = 0; nulls < 128; ++nulls) {
                            Call c = good;
                            c.n = n, c.m = m, c.object_max = object_max, c.max_frames = mf;
                            if (nulls & 1) c.tr = 0;
                            if (nulls & 2) c.slots = 0;
                            if (nulls & 4) c.wire = 0;
                            if (nulls & 8) c.off = 0;
                            if (nulls & 16) c.len = 0;
                            if (nulls & 32) c.result = 0;
                            if (nulls & 64) c.frame_status = 0;
                            same(c, open);
                        }
        /* the result array walks across the offsets, the lengths and the slots; without a list there is nothing to meet */
        for (uint32_t m : {1u, 2u, 5u})
            for (uint64_t result = 0x1000 - 130; result <= 0x1000 + 220; ++result)
                for (uint64_t slots : {(uint64_t)0x1000 + 120, (uint64_t)0}) {
                    Call c = good;
                    c.n = 8, c.m = m, c.off = 0x1000, c.len = 0x1000 + 60, c.slots = slots, c.result = result;
                    same(c, open);
                }
        /* the frame statuses walk across all four, under the call's cap and under the object's */
        for (uint32_t m : {1u, 3u})
            for (uint32_t mf : {0u, 1u, 7u, 40u})
                for (uint64_t fs = 0x1000 - 50; fs <= 0x1000 + 300; ++fs)
                    for (uint64_t slots : {(uint64_t)0x1000 + 120, (uint64_t)0}) {
                        Call c = good;
                        c.n = 8, c.m = m, c.object_max = 40, c.max_frames = mf, c.off = 0x1000, c.len = 0x1000 + 60, c.slots = slots;
                        c.result = 0x1000 + 180, c.frame_status = fs;
                        same(c, open);
                    }
        /* touching but not meeting, and one byte in; the ranges are m long, the result's entries 16 or 24 bytes */
        const uint64_t rb = open ? 24 : 16;
        for (uint32_t m : {1u, 3u, 67u}) {
            Call c = good;
            c.m = m;
            for (const auto &a : {std::pair<uint64_t, uint64_t>{c.off, 8}, {c.len, 4}, {c.slots, 4}}) {
                Call d = c;
                d.result = a.first + a.second * m;
                expect(d, open, OK, "touching above");
                d.result = a.first + a.second * m - 1;
                expect(d, open, BAD, "one byte in from above");
                d.result = a.first - rb * m;
                expect(d, open, OK, "touching below");
                d.result = a.first - rb * m + 1;
                expect(d, open, BAD, "one byte in from below");
                d = c;
                d.frame_status = a.first + a.second * m;
                expect(d, open, OK, "statuses touching above");
                d.frame_status = a.first + a.second * m - 1;
                expect(d, open, open ? BAD : OK, "statuses one byte in from above");
                d.frame_status = a.first - 64;
                expect(d, open, OK, "statuses touching below");
                d.frame_status = a.first - 63;
                expect(d, open, open ? BAD : OK, "statuses one byte in from below");
                d.max_frames = 63; /* the call's cap, not the object's */
                expect(d, open, OK, "statuses under the call's cap");
            }
            Call d = c;
            d.frame_status = c.result + rb * m - 1;
            expect(d, open, open ? BAD : OK, "statuses in the result");
            d.frame_status = c.result + rb * m;
            expect(d, open, OK, "statuses after the result");
            d = c;
            d.slots = 0;
            d.result = c.slots; /* no list given: nothing there to meet */
            expect(d, open, OK, "no list");
            d.frame_status = c.slots + 1;
            expect(d, open, open ? BAD : OK, "no list, statuses in the result");
        }
        /* the order, spelled out: each earlier rule wins over every later one */
        Call c = {0, 4, 64, 0, 0, 0, 0, 0, 0, 0, 0};
        expect(c, open, BAD, "NULL tr before m == 0");
        c.tr = 0x10, c.max_frames = 99;
        expect(c, open, OK, "m == 0 before the pointers and the cap");
        c.n = 0;
        expect(c, open, OK, "m == 0 on n == 0");
        c = good, c.n = 2, c.wire = 0;
        expect(c, open, BAD, "m > n");
        c = good, c.n = 0, c.m = 1;
        expect(c, open, BAD, "m > n on n == 0");
        c = good, c.max_frames = 65, c.result = c.off;
        expect(c, open, BAD, "the cap");
        c = good, c.max_frames = 64;
        expect(c, open, OK, "the object's cap itself");
        c = good, c.slots = 0;
        expect(c, open, OK, "a NULL list is allowed");
        c = good, c.frame_status = 0;
        expect(c, open, open ? BAD : OK, "the seal has no frame statuses");
        /* the edges of the arithmetic: nothing wraps */
        const uint32_t NMAX = 0xffffffffu;
        c = good, c.n = NMAX, c.m = 1, c.slots = MAXC - 3;
        expect(c, open, OK, "a list at the top of memory");
        c.result = MAXC - 3 - rb + 1;
        expect(c, open, BAD, "the result against it");
        c.result = MAXC - 3 - rb;
        expect(c, open, OK, "the result below it");
        c = good, c.n = NMAX, c.m = NMAX, c.off = 0x1000, c.len = 0x1000 + 8ull * NMAX, c.result = 0x1000 + 12ull * NMAX;
        c.slots = c.result + rb * NMAX, c.frame_status = c.slots + 4ull * NMAX, c.object_max = 0x80000000u, c.wire = 0x10;
        expect(c, open, OK, "2^32 - 1 entries packed");
        c.slots -= 1;
        expect(c, open, BAD, "2^32 - 1 entries, one byte in");
    }
}

int main(int argc, char **argv)
{
    run_window();
    run_walk();
    run_rules();
    for (int a = 1; a < argc; a += 4) {
        if (a + 3 >= argc || strcmp(argv[a], "expect")) {
            fail("argument", argv[a]);
            break;
        }
        const uint64_t accepted = strtoull(argv[a + 1], nullptr, 10), counter = strtoull(argv[a + 2], nullptr, 10);
        TrReplay *w = (TrReplay *)calloc(1, sizeof(TrReplay));
        tr_replay_accept(w, accepted);
        const bool fresh = tr_replay_check(w, counter);
        free(w);
        ++g_checks;
        if (fresh != (atoi(argv[a + 3]) != 0)) fail("expect", std::string(argv[a + 1]) + " " + argv[a + 2] + " " + argv[a + 3]);
    }
    printf("transport_datagram_check: %ld checks %ld failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
