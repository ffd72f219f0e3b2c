/*
 * transport_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd transport_check; tests/test_transport_host.py).
 *
 * The host-only half of the device-resident transport sessions
 * (csrc/transport_plan.h) on the CPU under ASan/UBSan: the frame walk the
 * kernels of csrc/transport.hip compile, the cap across sessions, and the
 * argument checks of noise_aead_dev_transport_*.
 *
 *   stdin   one walk per line, six fields:
 *             stream-hex  start-nonce  budget  frames  consumed  stop
 *           ('-' is the empty stream; the numbers are decimal).  The stream
 *           is copied to a heap buffer of exactly its length, so that ASan
 *           sees any read outside it; tr_walk must give the three expected
 *           values, and the frames it emits must tile [0, consumed) with
 *           bodies of at least 16 bytes, numbered from 0.  The test feeds the
 *           cases of tests/transport_model.py.
 *   then    the cap (tr_cap) against numbering the frames one by one, and the
 *           argument rules against a byte-by-byte reading of the header
 *           comment, over never-dereferenced pointers.
 *
 * Output: the last line "transport_check: <walks> walks <checks> checks
 * <failures> failures".
 */
#include "../csrc/transport_plan.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace na;

static long g_checks, g_failures;

static void fail(const char *what, const std::string &detail)
{
    if (++g_failures <= 20) fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

static bool unhex(const std::string &s, std::vector<uint8_t> &out)
{
    auto nib = [](char c) { return c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1); };
    out.clear();
    if (s == "-") return true;
    if (s.size() % 2) return false;
    for (size_t i = 0; i < s.size(); i += 2) {
        const int h = nib(s[i]), l = nib(s[i + 1]);
        if (h < 0 || l < 0) return false;
        out.push_back((uint8_t)(h * 16 + l));
    }
    return true;
}

struct Recorder {
    std::vector<uint64_t> *v; /* k, body, L per frame */
    void operator()(uint64_t k, uint64_t body, uint32_t L) const
    {
        v->push_back(k);
        v->push_back(body);
        v->push_back(L);
    }
};

static long run_walks()
{
    long walks = 0;
    std::string line;
    int c;
    while ((c = getchar()) != EOF) {
        if (c != '\n') {
            line.push_back((char)c);
            continue;
        }
        if (line.empty()) continue;
        const size_t sp = line.find(' ');
        std::vector<uint8_t> bytes;
        uint64_t nonce, budget, frames, consumed;
        int stop;
        const bool ok = sp != std::string::npos && unhex(line.substr(0, sp), bytes) &&
                        sscanf(line.c_str() + sp, " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %d", &nonce, &budget,
                               &frames, &consumed, &stop) == 5;
        if (!ok) {
            fail("input", line.substr(0, 80));
            line.clear();
            continue;
        }
        ++walks;
        /* exactly the stream's bytes on the heap (an empty stream: a pointer that must not be read) */
        uint8_t *p = bytes.empty() ? nullptr : (uint8_t *)malloc(bytes.size());
        if (!bytes.empty()) memcpy(p, bytes.data(), bytes.size());
        std::vector<uint64_t> seen;
        const TrWalk w = tr_walk(p, bytes.size(), nonce, budget, Recorder{&seen});
        const TrWalk plain = tr_walk(p, bytes.size(), nonce, budget);
        char b[200];
        snprintf(b, sizeof b, "len %zu nonce %" PRIu64 " budget %" PRIu64 ": got %" PRIu64 " %" PRIu64 " %#x want %" PRIu64
                 " %" PRIu64 " %#x", bytes.size(), nonce, budget, w.frames, w.consumed, w.stop, frames, consumed, stop);
        if (w.frames != frames || w.consumed != consumed || w.stop != stop) fail("walk", b);
        if (plain.frames != w.frames || plain.consumed != w.consumed || plain.stop != w.stop) fail("walk without emit", b);
        uint64_t at = 0;
        bool tiles = seen.size() == 3 * w.frames;
        for (size_t k = 0; tiles && k < seen.size() / 3; ++k) {
            tiles = seen[3 * k] == k && seen[3 * k + 1] == at + 2 && seen[3 * k + 2] >= TR_MAC_LEN &&
                    p[at] * 256u + p[at + 1] == seen[3 * k + 2];
            at += 2 + seen[3 * k + 2];
        }
        if (!tiles || at != w.consumed || w.consumed > bytes.size()) fail("emitted frames", b);
        if (!bytes.empty() && memcmp(p, bytes.data(), bytes.size())) fail("stream written", b);
        free(p);
        line.clear();
    }
    if (!line.empty()) fail("input", "last line has no newline");
    return walks;
}

/* ---- the cap, by numbering the frames */

static void run_cap()
{
    for (uint64_t max_frames = 1; max_frames <= 6; ++max_frames)
        for (uint64_t base = 0; base <= 8; ++base)
            for (uint64_t count = 0; count <= 8; ++count) {
                /* frames base .. base + count - 1; those below max_frames are processed */
                uint64_t below = 0;
                bool any_not = false;
                for (uint64_t f = base; f < base + count; ++f) {
                    if (f < max_frames) ++below;
                    else any_not = true;
                }
                /* a session with no frame of its own is cut when a frame numbered max_frames exists before it */
                const bool want_cut = any_not || (count == 0 && base > max_frames);
                bool cut;
                const uint64_t budget = tr_cap(base, count, max_frames, &cut);
                ++g_checks;
                if (cut != want_cut || budget != below) {
                    char b[160];
                    snprintf(b, sizeof b, "base %" PRIu64 " count %" PRIu64 " max %" PRIu64 ": budget %" PRIu64 " cut %d",
                             base, count, max_frames, budget, (int)cut);
                    fail("tr_cap", b);
                }
            }
    /* the edges of the arithmetic */
    const uint64_t TOP = ~0ull;
    struct { uint64_t base, count, max, budget; bool cut; } edge[] = {
        {TOP - 5, 5, 1u << 31, 0, true},       {TOP, 0, 1u << 31, 0, true},  {0, TOP, 1u << 31, 1u << 31, true},
        {(1u << 31) - 1, TOP, 1u << 31, 1, true}, {1u << 31, 0, 1u << 31, 0, false}, {0, 1u << 31, 1u << 31, 1u << 31, false},
        {1, 1u << 31, 1u << 31, (1u << 31) - 1, true},
    };
    for (const auto &e : edge) {
        bool cut;
        const uint64_t budget = tr_cap(e.base, e.count, e.max, &cut);
        ++g_checks;
        if (budget != e.budget || cut != e.cut) fail("tr_cap edge", std::to_string(e.base) + " " + std::to_string(e.count));
    }
}

/* ---- the argument rules, restated byte by byte */

typedef unsigned __int128 u128;

static bool bytes_meet(uint64_t a, u128 a_bytes, uint64_t b, u128 b_bytes)
{
    if (a_bytes > 4096 || b_bytes > 4096) { /* too many to count: the ranges as intervals */
        return a_bytes && b_bytes && (u128)a < (u128)b + b_bytes && (u128)b < (u128)a + a_bytes;
    }
    for (u128 x = a; x < (u128)a + a_bytes; ++x)
        if (x >= b && x < (u128)b + b_bytes) return true;
    return false;
}

static int rules_new(uint64_t out, int cipher, int role, uint32_t n, uint64_t k1, uint64_t k2, uint32_t max_frames)
{
    if (cipher != NOISE_CIPHER_CHACHAPOLY && cipher != NOISE_CIPHER_AESGCM) return NOISE_ERROR_UNKNOWN_ID;
    if (role != NOISE_ROLE_INITIATOR && role != NOISE_ROLE_RESPONDER) return NOISE_ERROR_INVALID_PARAM;
    if (!out || !k1 || !k2) return NOISE_ERROR_INVALID_PARAM;
    if (n > 0 && (max_frames == 0 || max_frames > 2147483648u)) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

static int rules_call(uint64_t tr, uint32_t n, uint64_t wire, uint64_t off, uint64_t len, uint64_t result)
{
    if (!tr || !wire || !off || !len || !result) return NOISE_ERROR_INVALID_PARAM;
    if (bytes_meet(result, (u128)16 * n, off, (u128)8 * n) || bytes_meet(result, (u128)16 * n, len, (u128)4 * n))
        return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

static const void *ptr(uint64_t v) { return (const void *)(uintptr_t)v; }

static void expect_new(uint64_t out, int cipher, int role, uint32_t n, uint64_t k1, uint64_t k2, uint32_t max_frames)
{
    ++g_checks;
    const int want = rules_new(out, cipher, role, n, k1, k2, max_frames);
    const int got = tr_check_new(ptr(out), cipher, role, n, ptr(k1), ptr(k2), max_frames);
    if (got != want) {
        char b[200];
        snprintf(b, sizeof b, "out %#" PRIx64 " cipher %#x role %#x n %u k1 %#" PRIx64 " k2 %#" PRIx64 " max %u: got %#x want %#x",
                 out, cipher, role, n, k1, k2, max_frames, got, want);
        fail("tr_check_new", b);
    }
}

static void expect_call(int want, uint64_t tr, uint32_t n, uint64_t wire, uint64_t off, uint64_t len, uint64_t result)
{
    ++g_checks;
    const int got = tr_check_call(ptr(tr), n, ptr(wire), ptr(off), ptr(len), ptr(result));
    if (got != want) {
        char b[200];
        snprintf(b, sizeof b, "tr %#" PRIx64 " n %u wire %#" PRIx64 " off %#" PRIx64 " len %#" PRIx64 " result %#" PRIx64
                 ": got %#x want %#x", tr, n, wire, off, len, result, got, want);
        fail("tr_check_call", b);
    }
}

static void run_rules()
{
    const int ciphers[] = {NOISE_CIPHER_CHACHAPOLY, NOISE_CIPHER_AESGCM, NOISE_CIPHER_NONE, NOISE_CIPHER_CATEGORY,
                           NOISE_ID('C', 3), NOISE_HASH_SHA256, -1};
    const int roles[] = {NOISE_ROLE_INITIATOR, NOISE_ROLE_RESPONDER, 0, NOISE_ID('R', 3), NOISE_ID('R', 0), 1, -1};
    const uint32_t counts[] = {0, 1, 67, 0xffffffffu};
    const uint32_t maxes[] = {0, 1, 2, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xffffffffu};
    for (int cipher : ciphers)
        for (int role : roles)
            for (uint32_t n : counts)
                for (uint32_t m : maxes)
                    for (int nulls = 0; nulls < 8; ++nulls)
                        expect_new(nulls & 1 ? 0 : 0x1000, cipher, role, n, nulls & 2 ? 0 : 0x2000, nulls & 4 ? 0 : 0x3000, m);
    /* a call: the result array walks across the offsets and the lengths */
    for (uint32_t n : {0u, 1u, 2u, 5u})
        for (uint64_t result = 0x1000 - 100; result <= 0x1000 + 160; ++result) {
            const uint64_t off = 0x1000, len = 0x1000 + 60;
            expect_call(rules_call(0x10, n, 0x9000, off, len, result), 0x10, n, 0x9000, off, len, result);
            for (int nulls = 1; nulls < 32; nulls += 5)
                expect_call(NOISE_ERROR_INVALID_PARAM, nulls & 1 ? 0 : 0x10, n, nulls & 2 ? 0 : 0x9000, nulls & 4 ? 0 : off,
                            nulls & 8 ? 0 : len, nulls & 16 ? 0 : result);
        }
    /* touching but not meeting, on both sides of both arrays, and one byte in */
    for (uint32_t n : {1u, 3u, 67u}) {
        const uint64_t off = 0x8000, len = 0x20000, far = 0x40000, tr = 0x10, wire = 0x90000;
        expect_call(NOISE_ERROR_NONE, tr, n, wire, off, len, off + 8ull * n);
        expect_call(NOISE_ERROR_INVALID_PARAM, tr, n, wire, off, len, off + 8ull * n - 1);
        expect_call(NOISE_ERROR_NONE, tr, n, wire, off, len, off - 16ull * n);
        expect_call(NOISE_ERROR_INVALID_PARAM, tr, n, wire, off, len, off - 16ull * n + 1);
        expect_call(NOISE_ERROR_NONE, tr, n, wire, off, len, len + 4ull * n);
        expect_call(NOISE_ERROR_INVALID_PARAM, tr, n, wire, off, len, len + 4ull * n - 1);
        expect_call(NOISE_ERROR_NONE, tr, n, wire, off, len, len - 16ull * n);
        expect_call(NOISE_ERROR_INVALID_PARAM, tr, n, wire, off, len, len - 16ull * n + 1);
        expect_call(NOISE_ERROR_INVALID_PARAM, tr, n, wire, off, len, off);
        expect_call(NOISE_ERROR_INVALID_PARAM, tr, n, wire, off, len, len);
        expect_call(NOISE_ERROR_NONE, tr, n, wire, off, len, far);
        /* the wire may hold anything, the result too: the streams are the caller's guarantee */
        expect_call(NOISE_ERROR_NONE, tr, n, far, off, len, far);
        /* n == 0: nothing can meet */
        expect_call(NOISE_ERROR_NONE, tr, 0, wire, off, len, off);
    }
    /* the edges of the arithmetic: nothing wraps */
    const uint32_t NMAX = 0xffffffffu;
    const uint64_t TOP = ~0ull;
    expect_call(NOISE_ERROR_INVALID_PARAM, 0x10, NMAX, 0x9000, 0x1000, TOP - 7, 0x2000);  /* 8 n bytes from 0x1000 */
    expect_call(NOISE_ERROR_NONE, 0x10, NMAX, 0x9000, 0x1000, 0x1000 + 8ull * NMAX, 0x1000 + 12ull * NMAX);
    expect_call(NOISE_ERROR_INVALID_PARAM, 0x10, NMAX, 0x9000, 0x1000, 0x1000 + 8ull * NMAX, 0x1000 + 12ull * NMAX - 1);
    expect_call(NOISE_ERROR_NONE, 0x10, 1, 0x9000, 0x1000, 0x2000, TOP - 15);
    expect_call(NOISE_ERROR_INVALID_PARAM, 0x10, 2, 0x9000, TOP - 15, 0x2000, TOP - 31);
    expect_call(NOISE_ERROR_NONE, 0x10, 1, 0x9000, TOP - 15, 0x2000, TOP - 31);
}

int main()
{
    static_assert(sizeof(NoiseAeadTransportResult) == 16, "the result is 16 bytes");
    const long walks = run_walks();
    run_cap();
    run_rules();
    printf("transport_check: %ld walks %ld checks %ld failures\n", walks, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
