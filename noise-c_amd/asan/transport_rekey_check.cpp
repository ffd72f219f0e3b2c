/*
 * transport_rekey_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd transport_rekey_check; tests/test_transport_rekey_host.py).
 *
 * The host-only half of rekey on the device (header section 12) on the CPU
 * under ASan/UBSan:
 *   - the argument checks of noise_aead_dev_rekey (csrc/dispatch.h check_rekey)
 *     and noise_aead_dev_transport_rekey (csrc/transport_plan.h tr_check_rekey)
 *     against a byte-by-byte reading of the header text, in the stated order,
 *     over never-dereferenced pointers: every order of causes, the exact
 *     in-place exception, ranges that touch but do not meet;
 *   - tr_rekey_directions, the one rule by which every kernel picks an entry's
 *     directions, over all 4 x 4 x {mask given, not given} cases (and the mask
 *     bytes with high bits set), the mask on a heap buffer of exactly its
 *     length so that ASan sees a read outside it;
 *   - the bytes of REKEY's counter blocks: the ChaCha20 counter and IV words
 *     and the two AES CTR blocks, against the bytes the header spells out.
 *
 * An argument "expect <directions> <which, or -1 for no mask> <want>" adds one
 * expectation of the caller's about tr_rekey_directions.  The test passes a
 * wrong one to see the program compare.
 *
 * Output: the last line "transport_rekey_check: <checks> checks <failures>
 * failures".
 */
#include "../csrc/dispatch.h"
#include "../csrc/transport_plan.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace na;

static long g_checks, g_failures;

static void fail(const char *what, const std::string &detail)
{
    if (++g_failures <= 20) fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

static const int OK = NOISE_ERROR_NONE, BAD = NOISE_ERROR_INVALID_PARAM, UNKNOWN = NOISE_ERROR_UNKNOWN_ID;

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

/* ---- the argument rules, restated byte by byte from the header */

typedef unsigned __int128 u128_t;

static bool bytes_meet(uint64_t a, u128_t a_bytes, uint64_t b, u128_t b_bytes)
{
    if (a_bytes > 8192 || b_bytes > 8192) /* too many to count: the ranges as intervals */
        return a_bytes && b_bytes && (u128_t)a < (u128_t)b + b_bytes && (u128_t)b < (u128_t)a + a_bytes;
    for (u128_t x = a; x < (u128_t)a + a_bytes; ++x)
        if (x >= b && x < (u128_t)b + b_bytes) return true;
    return false;
}

static int rules_rekey(int cipher, uint64_t keys, uint32_t n, uint64_t out)
{
    if (cipher != NOISE_CIPHER_CHACHAPOLY && cipher != NOISE_CIPHER_AESGCM) return UNKNOWN;
    if (n == 0) return OK;
    if (!keys || !out) return BAD;
    if (out == keys) return OK; /* exactly in place */
    if (bytes_meet(out, (u128_t)32 * n, keys, (u128_t)32 * n)) return BAD;
    return OK;
}

static int rules_transport_rekey(uint64_t tr, uint32_t n, uint32_t m, uint32_t directions)
{
    if (!tr) return BAD;
    if (m == 0) return OK;
    if (m > n) return BAD;
    if (directions == 0 || directions > 3) return BAD;
    return OK;
}

static void expect_rekey(int want, int cipher, uint64_t keys, uint32_t n, uint64_t out)
{
    char b[160];
    snprintf(b, sizeof b, "cipher %#x keys %#" PRIx64 " n %u out %#" PRIx64, cipher, keys, n, out);
    expect("check_rekey", check_rekey(cipher, ptr(keys), n, ptr(out)), want, b);
}

static void expect_transport(int want, uint64_t tr, uint32_t n, uint32_t m, uint32_t directions)
{
    char b[160];
    snprintf(b, sizeof b, "tr %#" PRIx64 " n %u m %u directions %#x", tr, n, m, directions);
    expect("tr_check_rekey", tr_check_rekey(ptr(tr), n, m, directions), want, b);
}

static void run_rules()
{
    const int ciphers[] = {NOISE_CIPHER_CHACHAPOLY, NOISE_CIPHER_AESGCM, NOISE_CIPHER_NONE, NOISE_ID('C', 3), -1};
    /* every combination of causes: the cipher, n, the NULLs, the ranges */
    for (int cipher : ciphers)
        for (uint32_t n : {0u, 1u, 2u, 67u, 0xffffffffu})
            for (uint64_t keys : {(uint64_t)0, (uint64_t)0x100000})
                for (uint64_t out : {(uint64_t)0, (uint64_t)0x100000, (uint64_t)0x100001, (uint64_t)0x900000000000ull})
                    expect_rekey(rules_rekey(cipher, keys, n, out), cipher, keys, n, out);
    /* the output walks across the keys: in place is fine, every other meeting is not */
    for (int cipher : {NOISE_CIPHER_CHACHAPOLY, NOISE_CIPHER_AESGCM})
        for (uint32_t n : {1u, 2u, 5u, 67u}) {
            const uint64_t keys = 0x100000;
            for (uint64_t out = keys - 32ull * n - 3; out <= keys + 32ull * n + 3; ++out)
                expect_rekey(rules_rekey(cipher, keys, n, out), cipher, keys, n, out);
            /* touching but not meeting, one byte in, and exactly in place */
            expect_rekey(OK, cipher, keys, n, keys + 32ull * n);
            expect_rekey(BAD, cipher, keys, n, keys + 32ull * n - 1);
            expect_rekey(OK, cipher, keys, n, keys - 32ull * n);
            expect_rekey(BAD, cipher, keys, n, keys - 32ull * n + 1);
            expect_rekey(OK, cipher, keys, n, keys);
            expect_rekey(BAD, cipher, keys, n, keys + 1);
            expect_rekey(BAD, cipher, keys, n, keys - 1);
            expect_rekey(n == 1 ? OK : BAD, cipher, keys, n, keys + 32); /* a whole key off is still a meeting */
        }
    /* the order, spelled out: each earlier rule wins over every later one */
    expect_rekey(UNKNOWN, NOISE_CIPHER_NONE, 0, 0, 0);                    /* the cipher before n == 0 */
    expect_rekey(UNKNOWN, NOISE_ID('C', 3), 0, 4, 0);                     /* ... and before the NULLs */
    expect_rekey(UNKNOWN, NOISE_ID('D', 1), 0x1000, 4, 0x1001);           /* ... and before the ranges */
    expect_rekey(OK, NOISE_CIPHER_AESGCM, 0, 0, 0);                       /* n == 0 before the NULLs */
    expect_rekey(OK, NOISE_CIPHER_CHACHAPOLY, 0x1000, 0, 0x1001);         /* n == 0 before the ranges */
    expect_rekey(BAD, NOISE_CIPHER_CHACHAPOLY, 0, 1, 0);                  /* NULL == NULL is not "in place" */
    expect_rekey(BAD, NOISE_CIPHER_AESGCM, 0, 1, 0x1000);
    expect_rekey(BAD, NOISE_CIPHER_AESGCM, 0x1000, 1, 0);
    /* the edges of the arithmetic: nothing wraps */
    const uint64_t TOP = ~0ull;
    const uint32_t NMAX = 0xffffffffu;
    expect_rekey(OK, NOISE_CIPHER_CHACHAPOLY, TOP - 31, 1, 0x1000);
    expect_rekey(OK, NOISE_CIPHER_CHACHAPOLY, TOP - 31, 1, TOP - 63);
    expect_rekey(BAD, NOISE_CIPHER_CHACHAPOLY, TOP - 31, 1, TOP - 62);
    expect_rekey(OK, NOISE_CIPHER_CHACHAPOLY, TOP - 31, 1, TOP - 31);
    expect_rekey(OK, NOISE_CIPHER_AESGCM, 0x1000, NMAX, 0x1000 + 32ull * NMAX);
    expect_rekey(BAD, NOISE_CIPHER_AESGCM, 0x1000, NMAX, 0x1000 + 32ull * NMAX - 1);
    expect_rekey(OK, NOISE_CIPHER_AESGCM, 0x1000, NMAX, 0x1000);

    /* the table call: the object, m against n, the directions */
    const uint32_t dirs[] = {0, 1, 2, 3, 4, 5, 0x80000001u, 0xffffffffu};
    for (uint64_t tr : {(uint64_t)0, (uint64_t)0x10})
        for (uint32_t n : {0u, 1u, 67u, 0xffffffffu})
            for (uint32_t m : {0u, 1u, 66u, 67u, 68u, 0xfffffffeu, 0xffffffffu})
                for (uint32_t d : dirs) expect_transport(rules_transport_rekey(tr, n, m, d), tr, n, m, d);
    expect_transport(BAD, 0, 4, 0, 3);       /* NULL tr before m == 0 */
    expect_transport(OK, 0x10, 4, 0, 0);     /* m == 0 before the directions */
    expect_transport(OK, 0x10, 0, 0, 99);    /* m == 0 on n == 0 */
    expect_transport(BAD, 0x10, 4, 5, 0);    /* m > n, whatever the directions */
    expect_transport(BAD, 0x10, 4, 4, 0);
    expect_transport(BAD, 0x10, 4, 4, 4);
    expect_transport(OK, 0x10, 4, 4, 1);
    expect_transport(OK, 0x10, 4, 4, 2);
    expect_transport(OK, 0x10, 4, 1, 3);
    static_assert(NOISE_AEAD_REKEY_SEND == 1u && NOISE_AEAD_REKEY_RECEIVE == 2u, "bit 0 is send, bit 1 is receive");
}

/* ---- the direction rule */

static void direction_case(uint32_t directions, int which, uint32_t want, const char *what = "tr_rekey_directions")
{
    /* the mask: m bytes on the heap with the case's byte last, so that entry m - 1 reads the buffer's end */
    for (uint32_t m : {1u, 5u}) {
        uint8_t *p = nullptr;
        if (which >= 0) {
            p = (uint8_t *)malloc(m);
            memset(p, 0xA5, m);
            p[m - 1] = (uint8_t)which;
        }
        const uint32_t got = tr_rekey_directions(directions, p, m - 1);
        ++g_checks;
        if (got != want) {
            char b[120];
            snprintf(b, sizeof b, "directions %u which %d entry %u: got %u want %u", directions, which, m - 1, got, want);
            fail(what, b);
        }
        free(p);
    }
}

static void run_directions()
{
    for (uint32_t d = 0; d < 4; ++d) {
        direction_case(d, -1, d); /* no mask: the call's directions */
        for (int w = 0; w < 4; ++w) {
            /* bit by bit: send if both say send, receive if both say receive */
            const uint32_t want = ((d & 1) && (w & 1) ? 1u : 0u) | ((d & 2) && (w & 2) ? 2u : 0u);
            direction_case(d, w, want);
            direction_case(d, w | 0xFC, want); /* the other bits of the byte say nothing */
        }
        direction_case(d, 0xFF, d);
    }
}

/* ---- the counter blocks */

static void run_blocks()
{
    /* ChaCha20 state words 12..15 as the block function lays them out, little-endian: counter 1, IV 2^64 - 1 */
    const uint32_t words[4] = {TR_REKEY_CHACHA_COUNTER, 0, TR_REKEY_CHACHA_IV_LO, TR_REKEY_CHACHA_IV_HI};
    uint8_t got[16];
    for (int w = 0; w < 4; ++w)
        for (int b = 0; b < 4; ++b) got[4 * w + b] = (uint8_t)(words[w] >> (8 * b));
    const uint8_t chacha[16] = {1, 0, 0, 0, 0, 0, 0, 0, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff};
    ++g_checks;
    if (memcmp(got, chacha, 16)) fail("blocks", "the ChaCha20 counter and IV");
    /* AES: 00000000 || FF x 8 || 00000002, then ... 00000003; words big-endian */
    for (uint32_t blk = 0; blk < 2; ++blk) {
        for (uint32_t w = 0; w < 4; ++w)
            for (int b = 0; b < 4; ++b) got[4 * w + b] = (uint8_t)(tr_rekey_aes_word(blk, w) >> (24 - 8 * b));
        const uint8_t aes[16] = {0, 0, 0, 0, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0, 0, 0, (uint8_t)(2 + blk)};
        ++g_checks;
        if (memcmp(got, aes, 16)) fail("blocks", "AES CTR block " + std::to_string(blk));
    }
    /* both are J0's successors for the nonce the CipherState never uses */
    ++g_checks;
    if ((((uint64_t)TR_REKEY_CHACHA_IV_HI << 32) | TR_REKEY_CHACHA_IV_LO) != TR_NONCE_LIMIT) fail("blocks", "the IV is not 2^64 - 1");
}

int main(int argc, char **argv)
{
    run_rules();
    run_directions();
    run_blocks();
    for (int a = 1; a < argc; a += 4) {
        if (a + 3 >= argc || strcmp(argv[a], "expect")) {
            fail("argument", argv[a]);
            break;
        }
        const long d = strtol(argv[a + 1], nullptr, 10), w = strtol(argv[a + 2], nullptr, 10), want = strtol(argv[a + 3], nullptr, 10);
        if (d < 0 || d > 3 || w < -1 || w > 255) {
            fail("argument", std::string(argv[a + 1]) + " " + argv[a + 2]);
            break;
        }
        direction_case((uint32_t)d, (int)w, (uint32_t)want, "expect");
    }
    printf("transport_rekey_check: %ld checks %ld failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
