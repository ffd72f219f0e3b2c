/*
 * handshake_ragged_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd handshake_ragged_check;
 * tests/test_handshake_ragged_host.py).
 *
 * The per-session half of the ragged handshake calls
 * (csrc/handshake_plan.h) on the CPU under ASan/UBSan.
 *
 *   stdout  hs_session_len — the source the kernels run — for every
 *           (overhead, length) with overhead in {0, 16, 32, 48, 64, 96, 112}
 *           and length in 0..300 and 65400..65600, both directions, a line
 *             len <W|R> <overhead> <length> <refused> <other>
 *           which the test compares with the model's rule
 *           (tests/handshake_ragged_model.py).
 *   then    hs_check_write_ragged and hs_check_read_ragged against a
 *           byte-by-byte reading of the header's list, in its order: every
 *           combination of NULL and given pointers, every action, n in 0..3,
 *           and the output length array slid over the arrays the call reads,
 *           with the arrays marked byte by byte; pointers are never
 *           dereferenced.
 *
 * The last line: "handshake_ragged_check: <lens> lens <checks> checks
 * <failures> failures".
 */
#include "../csrc/handshake_plan.h"

#include <cinttypes>
#include <cstdio>
#include <set>
#include <string>

using namespace na;

static long g_lens, g_checks, g_failures;

static void fail(const char *what, const std::string &detail)
{
    if (++g_failures <= 20) fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

static void print_lens()
{
    const uint32_t overheads[] = {0, 16, 32, 48, 64, 96, 112};
    for (int write = 0; write < 2; ++write)
        for (uint32_t over : overheads)
            for (uint32_t len = 0; len <= 65600; len = (len == 300 ? 65400 : len + 1)) {
                const HsLen r = hs_session_len(over, len, write != 0);
                printf("len %c %u %u %d %u\n", write ? 'W' : 'R', over, len, r.refused, r.other);
                ++g_lens;
            }
    /* lengths no 16-bit field holds: nothing wraps */
    for (uint32_t len : {65536u, 0x7FFFFFFFu, 0xFFFFFFF0u, 0xFFFFFFFFu})
        for (int write = 0; write < 2; ++write) {
            const HsLen r = hs_session_len(48, len, write != 0);
            ++g_checks;
            if (!r.refused || r.other) fail("wide length", std::to_string(len));
        }
}

/* ---- the header's list, byte by byte */

typedef std::set<uint64_t> Bytes;

static Bytes mark(uint64_t p, uint64_t bytes)
{
    Bytes b;
    for (uint64_t j = 0; p && j < bytes; ++j) b.insert(p + j);
    return b;
}

static bool meets(const Bytes &a, const Bytes &b)
{
    for (uint64_t x : a)
        if (b.count(x)) return true;
    return false;
}

static const void *ptr(uint64_t v) { return (const void *)(uintptr_t)v; }

/* data, off, len of the input side; data, off of the output side; the output length array */
struct Args {
    uint64_t hs, in, in_off, in_len, out, out_off, out_len;
};

static int rule(bool write, int action, uint32_t n, const Args &a)
{
    if (!a.hs) return NOISE_ERROR_INVALID_PARAM;
    if (action != (write ? NOISE_ACTION_WRITE_MESSAGE : NOISE_ACTION_READ_MESSAGE)) return NOISE_ERROR_INVALID_STATE;
    if (!n) return NOISE_ERROR_NONE;
    const bool triple_null = !a.in && !a.in_off && !a.in_len, triple_given = a.in && a.in_off && a.in_len;
    if (!a.out || !a.out_off || !a.out_len) return NOISE_ERROR_INVALID_PARAM;
    if (write ? !(triple_null || triple_given) : !triple_given) return NOISE_ERROR_INVALID_PARAM;
    const Bytes out = mark(a.out_len, 4ull * n);
    if (meets(out, mark(a.in_off, 8ull * n)) || meets(out, mark(a.out_off, 8ull * n)) || meets(out, mark(a.in_len, 4ull * n)))
        return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

static int call(bool write, int action, uint32_t n, const Args &a)
{
    /* write: payload -> msg; read: msg -> payload */
    return write ? hs_check_write_ragged(ptr(a.hs), action, n, ptr(a.in), ptr(a.in_off), ptr(a.in_len), ptr(a.out),
                                         ptr(a.out_off), ptr(a.out_len))
                 : hs_check_read_ragged(ptr(a.hs), action, n, ptr(a.in), ptr(a.in_off), ptr(a.in_len), ptr(a.out),
                                        ptr(a.out_off), ptr(a.out_len));
}

static void compare(bool write, int action, uint32_t n, const Args &a)
{
    const int want = rule(write, action, n, a), got = call(write, action, n, a);
    ++g_checks;
    if (got != want) {
        char d[240];
        snprintf(d, sizeof(d),
                 "write=%d action=%#x n=%u hs=%" PRIu64 " in=%" PRIu64 " in_off=%" PRIu64 " in_len=%" PRIu64 " out=%" PRIu64
                 " out_off=%" PRIu64 " out_len=%" PRIu64 ": got %#x want %#x",
                 write, action, n, a.hs, a.in, a.in_off, a.in_len, a.out, a.out_off, a.out_len, got, want);
        fail("ragged check", d);
    }
}

static void check_calls()
{
    const int actions[] = {NOISE_ACTION_WRITE_MESSAGE, NOISE_ACTION_READ_MESSAGE, NOISE_ACTION_SPLIT, NOISE_ACTION_NONE};
    /* the arrays far apart: every NULL pattern, every action, every n */
    const Args apart = {8, 1000, 2000, 3000, 4000, 5000, 6000};
    for (int write = 0; write < 2; ++write)
        for (int action : actions)
            for (uint32_t n = 0; n < 4; ++n)
                for (unsigned nulls = 0; nulls < 128; ++nulls) {
                    Args a = apart;
                    uint64_t *f[7] = {&a.hs, &a.in, &a.in_off, &a.in_len, &a.out, &a.out_off, &a.out_len};
                    for (int b = 0; b < 7; ++b)
                        if (nulls >> b & 1) *f[b] = 0;
                    compare(write != 0, action, n, a);
                }
    /* the output length array slid over each array the call reads; the data
       pointers may lie anywhere, over the arrays too: they are the caller's */
    for (int write = 0; write < 2; ++write) {
        const int action = write ? NOISE_ACTION_WRITE_MESSAGE : NOISE_ACTION_READ_MESSAGE;
        for (uint32_t n = 1; n < 4; ++n)
            for (uint64_t at = 60; at < 180; ++at) {
                Args a = {8, 1000, 100, 140, 4000, 64, at};
                compare(write != 0, action, n, a);
                a.in = at; /* the data on the length array: not the host's to refuse */
                a.out_len = 6000;
                compare(write != 0, action, n, a);
                if (write) {
                    a = {8, 0, 0, 0, 4000, 100, at}; /* no payload triple: only the message offsets are read */
                    compare(true, action, n, a);
                }
            }
    }
    /* at the edge of 64-bit arithmetic: 4n and 8n bytes never wrap */
    struct Edge { int got, want; const char *what; };
    const uint64_t top = ~0ull;
    const int W = NOISE_ACTION_WRITE_MESSAGE, R = NOISE_ACTION_READ_MESSAGE;
    const Edge edges[] = {
        {hs_check_write_ragged(ptr(8), W, 0xFFFFFFFFu, ptr(64), ptr(top - 15), ptr(1ull << 60), ptr(64), ptr(1ull << 40), ptr(16)), 0,
         "offsets that end past 2^64 do not reach a low output"},
        {hs_check_write_ragged(ptr(8), W, 0xFFFFFFFFu, ptr(64), ptr(1ull << 50), ptr(1 << 20), ptr(64), ptr(1ull << 40), ptr(top - 3)),
         0, "an output that ends past 2^64 does not reach low arrays"},
        {hs_check_read_ragged(ptr(8), R, 0xFFFFFFFFu, ptr(64), ptr(top - 100), ptr(1 << 20), ptr(64), ptr(1ull << 40), ptr(top - 50)),
         NOISE_ERROR_INVALID_PARAM, "high offsets under a high output"},
        {hs_check_read_ragged(ptr(8), R, 2, ptr(64), ptr(100), ptr(116), ptr(64), ptr(124), ptr(140)), 0, "arrays that touch"},
        {hs_check_read_ragged(ptr(8), R, 2, ptr(64), ptr(100), ptr(116), ptr(64), ptr(124), ptr(139)), NOISE_ERROR_INVALID_PARAM,
         "the last byte of the payload offsets"},
        {hs_check_read_ragged(nullptr, R, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), NOISE_ERROR_INVALID_PARAM, "no object"},
        {hs_check_read_ragged(ptr(8), W, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), NOISE_ERROR_INVALID_STATE,
         "the state before n == 0"},
        {hs_check_read_ragged(ptr(8), R, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), 0, "n == 0 takes NULL pointers"},
    };
    for (const Edge &e : edges) {
        ++g_checks;
        if (e.got != e.want) fail("edge", e.what);
    }
}

int main()
{
    print_lens();
    check_calls();
    printf("handshake_ragged_check: %ld lens %ld checks %ld failures\n", g_lens, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
