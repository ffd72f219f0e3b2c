/*
 * transport_table_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd transport_table_check; tests/test_transport_table_host.py).
 *
 * The session table's host-only half (csrc/transport_plan.h, header section
 * 10) on the CPU under ASan/UBSan:
 *   - tr_slot, the one function through which every kernel resolves the slot
 *     of a call's entry, over slot lists on heap buffers of exactly their
 *     length (so that ASan sees a read outside one), with the values n - 1, n
 *     and 2^32 - 1 among them, and over the NULL list;
 *   - the argument checks of _new_unkeyed, _set_keys, _clear_keys and the _of
 *     calls against a byte-by-byte reading of the header text, in the stated
 *     order, over never-dereferenced pointers.
 *
 * An argument "expect <n> <slot> <0|1>" adds one expectation of the caller's:
 * tr_slot of the one-entry list {slot} on n slots must say in range (1) or
 * not (0).  The test passes a wrong one to see the program compare.
 *
 * Output: the last line "transport_table_check: <checks> checks <failures>
 * failures".
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

/* ---- tr_slot */

static void slot_list(const std::vector<uint32_t> &list, uint32_t n)
{
    /* exactly the list's entries on the heap */
    uint32_t *p = (uint32_t *)malloc(list.size() * sizeof(uint32_t));
    memcpy(p, list.data(), list.size() * sizeof(uint32_t));
    for (uint32_t j = 0; j < list.size(); ++j) {
        uint32_t i = 0xA5A5A5A5u;
        const bool in = tr_slot(p, j, n, &i);
        ++g_checks;
        if (i != list[j] || in != ((uint64_t)list[j] < (uint64_t)n)) {
            char b[120];
            snprintf(b, sizeof b, "n %u entry %u of %zu: slot %u, got %u in range %d", n, j, list.size(), list[j], i, (int)in);
            fail("tr_slot", b);
        }
    }
    if (memcmp(p, list.data(), list.size() * sizeof(uint32_t))) fail("tr_slot", "list written");
    free(p);
}

static void run_slots()
{
    const uint32_t TOP = 0xffffffffu;
    for (uint32_t n : {0u, 1u, 2u, 64u, 67u, 65536u, 0x80000000u, TOP}) {
        slot_list({n - 1}, n); /* n == 0: 2^32 - 1 */
        slot_list({n}, n);
        slot_list({TOP}, n);
        slot_list({n - 1, n, TOP, 0, n / 2, n + 1, 0x7fffffffu, 0x80000000u}, n);
        /* a scrambled list over every slot, with the three edge values at its ends */
        if (n >= 2 && n <= 67) {
            std::vector<uint32_t> all;
            for (uint32_t j = 0; j < n; ++j) all.push_back((29 * j + 5) % n);
            all.insert(all.begin(), n);
            all.push_back(TOP);
            all.push_back(n - 1);
            slot_list(all, n);
        }
        /* the NULL list: entry j is slot j, and no list is read */
        for (uint32_t j : {0u, 1u, n - 1, n, n + 1, TOP}) {
            uint32_t i = 0xA5A5A5A5u;
            const bool in = tr_slot(nullptr, j, n, &i);
            ++g_checks;
            if (i != j || in != (j < n)) fail("tr_slot NULL list", std::to_string(n) + " " + std::to_string(j));
        }
    }
}

/* ---- the argument rules, restated byte by byte from the header */

typedef unsigned __int128 u128;

static bool bytes_meet(uint64_t a, u128 a_bytes, uint64_t b, u128 b_bytes)
{
    if (a_bytes > 4096 || b_bytes > 4096) /* too many to count: the ranges as intervals */
        return a_bytes && b_bytes && (u128)a < (u128)b + b_bytes && (u128)b < (u128)a + a_bytes;
    for (u128 x = a; x < (u128)a + a_bytes; ++x)
        if (x >= b && x < (u128)b + b_bytes) return true;
    return false;
}

static const int OK = NOISE_ERROR_NONE, BAD = NOISE_ERROR_INVALID_PARAM;

static int rules_new_unkeyed(uint64_t out, int cipher, int role, uint32_t n, uint32_t max_frames)
{
    if (cipher != NOISE_CIPHER_CHACHAPOLY && cipher != NOISE_CIPHER_AESGCM) return NOISE_ERROR_UNKNOWN_ID;
    if (role != NOISE_ROLE_INITIATOR && role != NOISE_ROLE_RESPONDER) return BAD;
    if (!out) return BAD;
    if (n > 0 && (max_frames == 0 || max_frames > 2147483648u)) return BAD;
    return OK;
}

static int rules_set_keys(uint64_t tr, uint32_t n, uint64_t slots, uint32_t m, uint64_t k1, uint64_t k2)
{
    if (!tr) return BAD;
    if (m == 0) return OK;
    if (m > n) return BAD;
    if (!slots || !k1 || !k2) return BAD;
    return OK;
}

static int rules_clear_keys(uint64_t tr, uint32_t n, uint64_t slots, uint32_t m)
{
    if (!tr) return BAD;
    if (m == 0) return OK;
    if (m > n) return BAD;
    if (!slots) return BAD;
    return OK;
}

static int rules_of(uint64_t tr, uint32_t n, uint32_t object_max, uint64_t slots, uint32_t m, uint32_t max_frames,
                    uint64_t wire, uint64_t off, uint64_t len, uint64_t result)
{
    if (!tr) return BAD;
    if (m == 0) return OK;
    if (m > n) return BAD;
    if (!slots || !wire || !off || !len || !result) return BAD;
    if (max_frames > object_max) return BAD;
    if (bytes_meet(result, (u128)16 * m, off, (u128)8 * m) || bytes_meet(result, (u128)16 * m, len, (u128)4 * m) ||
        bytes_meet(result, (u128)16 * m, slots, (u128)4 * m))
        return BAD;
    return OK;
}

static const void *ptr(uint64_t v) { return (const void *)(uintptr_t)v; }

static void expect(const char *what, int got, int want, const std::string &detail)
{
    ++g_checks;
    if (got != want) {
        char b[60];
        snprintf(b, sizeof b, ": got %#x want %#x", got, want);
        fail(what, detail + b);
    }
}

static void expect_of(int want, uint64_t tr, uint32_t n, uint32_t object_max, uint64_t slots, uint32_t m, uint32_t max_frames,
                      uint64_t wire, uint64_t off, uint64_t len, uint64_t result)
{
    char b[240];
    snprintf(b, sizeof b, "tr %#" PRIx64 " n %u object max %u slots %#" PRIx64 " m %u max %u wire %#" PRIx64 " off %#" PRIx64
             " len %#" PRIx64 " result %#" PRIx64, tr, n, object_max, slots, m, max_frames, wire, off, len, result);
    expect("tr_check_call_of", tr_check_call_of(ptr(tr), n, object_max, ptr(slots), m, max_frames, ptr(wire), ptr(off),
                                                ptr(len), ptr(result)), want, b);
}

static void run_rules()
{
    const int ciphers[] = {NOISE_CIPHER_CHACHAPOLY, NOISE_CIPHER_AESGCM, NOISE_CIPHER_NONE, NOISE_ID('C', 3), -1};
    const int roles[] = {NOISE_ROLE_INITIATOR, NOISE_ROLE_RESPONDER, 0, NOISE_ID('R', 3), 1};
    const uint32_t maxes[] = {0, 1, 64, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xffffffffu};
    for (int cipher : ciphers)
        for (int role : roles)
            for (uint32_t n : {0u, 1u, 67u, 0xffffffffu})
                for (uint32_t mf : maxes)
                    for (uint64_t out : {(uint64_t)0, (uint64_t)0x1000})
                        expect("tr_check_new_unkeyed", tr_check_new_unkeyed(ptr(out), cipher, role, n, mf),
                               rules_new_unkeyed(out, cipher, role, n, mf),
                               std::to_string(cipher) + " " + std::to_string(role) + " " + std::to_string(n) + " " +
                                   std::to_string(mf) + " " + std::to_string(out));
    /* _set_keys and _clear_keys: every combination of NULLs at every relation of m to n */
    const uint32_t ns[] = {0, 1, 67, 0xffffffffu};
    for (uint32_t n : ns)
        for (uint32_t m : {0u, 1u, 66u, 67u, 68u, 0xfffffffeu, 0xffffffffu})
            for (int nulls = 0; nulls < 16; ++nulls) {
                const uint64_t tr = nulls & 1 ? 0 : 0x10, slots = nulls & 2 ? 0 : 0x1000, k1 = nulls & 4 ? 0 : 0x2000,
                               k2 = nulls & 8 ? 0 : 0x3000;
                const std::string d = std::to_string(n) + " " + std::to_string(m) + " nulls " + std::to_string(nulls);
                expect("tr_check_set_keys", tr_check_set_keys(ptr(tr), n, ptr(slots), m, ptr(k1), ptr(k2)),
                       rules_set_keys(tr, n, slots, m, k1, k2), d);
                expect("tr_check_clear_keys", tr_check_clear_keys(ptr(tr), n, ptr(slots), m),
                       rules_clear_keys(tr, n, slots, m), d);
            }
    /* the order, spelled out: each earlier rule wins over every later one */
    expect("set_keys order", tr_check_set_keys(nullptr, 4, nullptr, 0, nullptr, nullptr), BAD, "NULL tr before m == 0");
    expect("set_keys order", tr_check_set_keys(ptr(0x10), 4, nullptr, 0, nullptr, nullptr), OK, "m == 0 before the pointers");
    expect("set_keys order", tr_check_set_keys(ptr(0x10), 0, nullptr, 0, nullptr, nullptr), OK, "m == 0 on n == 0");
    expect("set_keys order", tr_check_set_keys(ptr(0x10), 4, ptr(0x1000), 5, ptr(0x2000), ptr(0x3000)), BAD, "m > n");
    expect("clear_keys order", tr_check_clear_keys(nullptr, 4, nullptr, 0), BAD, "NULL tr before m == 0");
    expect("clear_keys order", tr_check_clear_keys(ptr(0x10), 4, nullptr, 0), OK, "m == 0 before the pointer");
    expect("clear_keys order", tr_check_clear_keys(ptr(0x10), 4, ptr(0x1000), 4), OK, "m == n");

    /* the _of calls: NULLs, m against n, the cap against the object's */
    for (uint32_t n : ns)
        for (uint32_t m : {0u, 1u, 67u, 68u, 0xffffffffu})
            for (uint32_t object_max : {1u, 64u, 0x80000000u})
                for (uint32_t mf : {0u, 1u, 64u, 65u, 0x80000000u, 0xffffffffu})
                    for (int nulls = 0; nulls < 64; ++nulls) {
                        const uint64_t tr = nulls & 1 ? 0 : 0x10, slots = nulls & 2 ? 0 : 0x100000, wire = nulls & 4 ? 0 : 0x9000000,
                                       off = nulls & 8 ? 0 : 0x200000, len = nulls & 16 ? 0 : 0x300000,
                                       result = nulls & 32 ? 0 : 0x400000;
                        expect_of(rules_of(tr, n, object_max, slots, m, mf, wire, off, len, result), tr, n, object_max, slots, m,
                                  mf, wire, off, len, result);
                    }
    /* the result array walks across the offsets, the lengths and the slots */
    for (uint32_t m : {1u, 2u, 5u})
        for (uint64_t result = 0x1000 - 100; result <= 0x1000 + 220; ++result) {
            const uint64_t off = 0x1000, len = 0x1000 + 60, slots = 0x1000 + 120;
            expect_of(rules_of(0x10, 8, 64, slots, m, 0, 0x9000, off, len, result), 0x10, 8, 64, slots, m, 0, 0x9000, off, len,
                      result);
        }
    /* touching but not meeting, on both sides of the three arrays, and one byte in; the ranges are m long, not n long */
    for (uint32_t m : {1u, 3u, 67u}) {
        const uint64_t off = 0x8000, len = 0x20000, slots = 0x30000, far = 0x40000, tr = 0x10, wire = 0x90000;
        const uint32_t n = 1000;
        for (const auto &a : {std::pair<uint64_t, uint64_t>{off, 8}, {len, 4}, {slots, 4}}) {
            expect_of(OK, tr, n, 64, slots, m, 64, wire, off, len, a.first + a.second * m);
            expect_of(BAD, tr, n, 64, slots, m, 64, wire, off, len, a.first + a.second * m - 1);
            expect_of(OK, tr, n, 64, slots, m, 64, wire, off, len, a.first - 16ull * m);
            expect_of(BAD, tr, n, 64, slots, m, 64, wire, off, len, a.first - 16ull * m + 1);
            expect_of(BAD, tr, n, 64, slots, m, 64, wire, off, len, a.first);
        }
        expect_of(OK, tr, n, 64, slots, m, 64, wire, off, len, far);
        expect_of(OK, tr, n, 64, slots, m, 64, far, off, len, far); /* the wire: the caller's guarantee */
        expect_of(BAD, tr, n, 64, slots, m, 65, wire, off, len, far);
        expect_of(BAD, tr, n, 64, slots, m, 65, wire, off, len, off); /* either way */
        expect_of(OK, tr, n, 64, slots, 0, 65, wire, off, len, off);  /* m == 0: before the cap and the ranges */
        expect_of(BAD, tr, m - 1, 64, slots, m, 0, wire, off, len, far);
        expect_of(OK, tr, m, 64, slots, m, 0, wire, off, len, far);
    }
    /* the order, spelled out */
    expect_of(BAD, 0, 4, 64, 0, 0, 0, 0, 0, 0, 0);            /* NULL tr before m == 0 */
    expect_of(OK, 0x10, 4, 64, 0, 0, 99, 0, 0, 0, 0);         /* m == 0 before the pointers and the cap */
    expect_of(OK, 0x10, 0, 64, 0, 0, 0, 0, 0, 0, 0);          /* m == 0 on n == 0 */
    expect_of(BAD, 0x10, 0, 64, 0x1000, 1, 0, 0x9000, 0x2000, 0x3000, 0x4000); /* m > n on n == 0 */
    /* the edges of the arithmetic: nothing wraps */
    const uint32_t NMAX = 0xffffffffu;
    const uint64_t TOP = ~0ull;
    expect_of(OK, 0x10, NMAX, 64, TOP - 3, 1, 0, 0x9000, 0x1000, 0x2000, 0x3000);
    expect_of(BAD, 0x10, NMAX, 64, TOP - 3, 1, 0, 0x9000, 0x1000, 0x2000, TOP - 15);
    expect_of(OK, 0x10, NMAX, 64, TOP - 3, 1, 0, 0x9000, 0x1000, 0x2000, TOP - 19);
    expect_of(OK, 0x10, NMAX, 64, 0x1000 + 28ull * NMAX, NMAX, 0, 0x9000, 0x1000, 0x1000 + 8ull * NMAX, 0x1000 + 12ull * NMAX);
    expect_of(BAD, 0x10, NMAX, 64, 0x1000 + 28ull * NMAX - 1, NMAX, 0, 0x9000, 0x1000, 0x1000 + 8ull * NMAX,
              0x1000 + 12ull * NMAX);
}

int main(int argc, char **argv)
{
    static_assert(sizeof(NoiseAeadTransportResult) == 16, "the result is 16 bytes");
    run_slots();
    run_rules();
    for (int a = 1; a < argc; a += 4) {
        if (a + 3 >= argc || strcmp(argv[a], "expect")) {
            fail("argument", argv[a]);
            break;
        }
        const uint32_t n = (uint32_t)strtoull(argv[a + 1], nullptr, 10), slot = (uint32_t)strtoull(argv[a + 2], nullptr, 10);
        uint32_t *p = (uint32_t *)malloc(sizeof(uint32_t));
        *p = slot;
        uint32_t i;
        const bool in = tr_slot(p, 0, n, &i);
        free(p);
        ++g_checks;
        if (in != (atoi(argv[a + 3]) != 0) || i != slot)
            fail("expect", std::string(argv[a + 1]) + " " + argv[a + 2] + " " + argv[a + 3]);
    }
    printf("transport_table_check: %ld checks %ld failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
