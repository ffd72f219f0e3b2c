/*
 * dh_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd dh_check; tests/test_dh_host.py).
 *
 * The X25519 code the GPU kernels run (csrc/fe25519.h) and the host checks of
 * noise_aead_dev_dh_calculate / _dh_public (csrc/dispatch.h check_dh) on the
 * CPU under ASan/UBSan.
 *
 *   stdin   one case per line, four hex fields of 32 bytes:
 *             private  public-value  shared  public-key
 *           shared must be X25519(private, public-value) and public-key
 *           X25519(private, 9); the test feeds tests/golden/x25519.json.
 *           A line "f25 <op> <a> <b> <result>" is one field operation instead:
 *           op is add, sub, mul, sq, freeze, invert or mul_small_<k> (decimal
 *           k < 2^26), a and b any 256-bit values (b is read by add, sub and
 *           mul only), result the canonical residue, each the hex of 32
 *           little-endian bytes.  The operation's raw output is frozen and
 *           compared; freeze's own output is compared as it is.  The test
 *           feeds every vector of tests/f25_cases.py.
 *   then    the argument rules against a byte-by-byte reading of the header:
 *           every small layout (pointers, strides, counts), the spans that
 *           touch without meeting, stride 0, n = 1, and values at the edges
 *           of 64-bit arithmetic, over never-dereferenced pointers.
 *
 * Output: "dh_check f25: <vectors> vectors <failures> failures", then the last
 * line "dh_check: <cases> cases <checks> checks <failures> failures" (cases
 * counts the X25519 lines, failures everything).
 */
#include "../csrc/dispatch.h"
#include "../csrc/fe25519.h"

#include <cinttypes>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace na;

static long g_checks, g_failures, g_f25, g_f25_failures;

static void fail(const char *what, const std::string &detail)
{
    if (++g_failures <= 20) fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

static bool unhex(const char *s, size_t len, std::vector<uint8_t> &out)
{
    auto nib = [](char c) { return c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1); };
    if (len != 64) return false;
    out.resize(32);
    for (int i = 0; i < 32; ++i) {
        const int h = nib(s[2 * i]), l = nib(s[2 * i + 1]);
        if (h < 0 || l < 0) return false;
        out[i] = (uint8_t)(h * 16 + l);
    }
    return true;
}

static std::string hex(const uint8_t *p)
{
    char b[65];
    for (int i = 0; i < 32; ++i) snprintf(b + 2 * i, 3, "%02x", p[i]);
    return b;
}

/* what one lane of x25519_batch<BASE> does, on heap buffers of exactly 32
   bytes so that ASan sees any access outside them */
template <bool BASE>
static std::vector<uint8_t> lane(const std::vector<uint8_t> &priv, const std::vector<uint8_t> &pub)
{
    std::vector<uint8_t> out(32, 0xA5);
    const F25 k = f25_load(priv.data());
    const F25 u = BASE ? f25_small(9) : f25_load(pub.data());
    f25_store(out.data(), x25519<BASE>(k, u));
    return out;
}

/* one "f25" line (after the word): what one lane of f25_op_batch does, then
   the freeze, again on heap buffers of exactly 32 bytes */
static void run_f25(const char *p)
{
    const char *const line = p;
    char op[32];
    std::vector<uint8_t> f[3];
    size_t len = 0;
    while (p[len] && p[len] != ' ' && p[len] != '\n') ++len;
    bool ok = len > 0 && len < sizeof op;
    if (ok) {
        memcpy(op, p, len);
        op[len] = 0;
        p += len;
    }
    for (int k = 0; k < 3 && ok; ++k) {
        while (*p == ' ') ++p;
        len = 0;
        while (p[len] && p[len] != ' ' && p[len] != '\n') ++len;
        ok = unhex(p, len, f[k]);
        p += len;
    }
    F25 r;
    bool frozen = false;
    if (ok) {
        const F25 a = f25_load(f[0].data()), b = f25_load(f[1].data());
        if (!strcmp(op, "add")) r = f25_add(a, b);
        else if (!strcmp(op, "sub")) r = f25_sub(a, b);
        else if (!strcmp(op, "mul")) r = f25_mul(a, b);
        else if (!strcmp(op, "sq")) r = f25_sq(a);
        else if (!strcmp(op, "invert")) r = f25_invert(a);
        else if (!strcmp(op, "freeze")) {
            r = f25_freeze(a);
            frozen = true;
        } else if (!strncmp(op, "mul_small_", 10)) {
            char *end;
            const unsigned long k = strtoul(op + 10, &end, 10);
            ok = end != op + 10 && !*end && k < (1ul << 26);
            if (ok) r = f25_mul_small(a, (uint32_t)k);
        } else
            ok = false;
    }
    if (!ok) {
        fail("input", std::string("f25 ") + line);
        return;
    }
    ++g_f25;
    std::vector<uint8_t> out(32, 0xA5);
    f25_store(out.data(), frozen ? r : f25_freeze(r));
    if (out != f[2]) {
        ++g_f25_failures;
        fail((std::string("f25 ") + op).c_str(), hex(f[0].data()) + " " + hex(f[1].data()) + " -> " + hex(out.data()));
    }
}

static long run_cases()
{
    long cases = 0;
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "f25 ", 4)) {
            run_f25(line + 4);
            continue;
        }
        std::vector<uint8_t> f[4];
        const char *p = line;
        bool ok = true;
        for (int k = 0; k < 4 && ok; ++k) {
            while (*p == ' ') ++p;
            size_t len = 0;
            while (p[len] && p[len] != ' ' && p[len] != '\n') ++len;
            ok = unhex(p, len, f[k]);
            p += len;
        }
        if (!ok) {
            if (line[0] != '\n') fail("input", line);
            continue;
        }
        ++cases;
        const std::vector<uint8_t> priv0 = f[0], pub0 = f[1];
        const std::vector<uint8_t> shared = lane<false>(f[0], f[1]);
        const std::vector<uint8_t> pk = lane<true>(f[0], f[1]);
        if (shared != f[2]) fail("calculate", hex(f[0].data()) + " " + hex(f[1].data()) + " -> " + hex(shared.data()));
        if (pk != f[3]) fail("public", hex(f[0].data()) + " -> " + hex(pk.data()));
        if (f[0] != priv0 || f[1] != pub0) fail("inputs written", hex(priv0.data()));
    }
    return cases;
}

/* ---- the argument rules, restated byte by byte */

static bool byte_in_span(u128 x, u128 ptr, u128 stride, uint32_t n)
{
    u128 end = ptr; /* [ptr, ptr + (n - 1) stride + 32), or [ptr, + 32) at stride 0 */
    for (uint32_t i = 1; i < n; ++i) end += stride;
    end += 32;
    return x >= ptr && x < end;
}

static int rules(int dh_id, uint64_t priv, uint64_t ps, bool has_pub, uint64_t pub, uint64_t us, uint32_t n,
                 uint64_t out)
{
    if (dh_id != NOISE_DH_CURVE25519) return NOISE_ERROR_UNKNOWN_ID;
    if (n == 0) return NOISE_ERROR_NONE;
    if (!priv || !out || (has_pub && !pub)) return NOISE_ERROR_INVALID_PARAM;
    if (ps >= 1 && ps <= 31) return NOISE_ERROR_INVALID_PARAM;
    if (has_pub && us >= 1 && us <= 31) return NOISE_ERROR_INVALID_PARAM;
    for (u128 x = out; x < (u128)out + (u128)32 * n; ++x) {
        if (byte_in_span(x, priv, ps, n)) return NOISE_ERROR_INVALID_PARAM;
        if (has_pub && byte_in_span(x, pub, us, n)) return NOISE_ERROR_INVALID_PARAM;
    }
    return NOISE_ERROR_NONE;
}

static void expect(int want, int dh_id, uint64_t priv, uint64_t ps, bool has_pub, uint64_t pub, uint64_t us,
                   uint32_t n, uint64_t out)
{
    ++g_checks;
    const int got = check_dh(dh_id, (const void *)(uintptr_t)priv, ps, has_pub, (const void *)(uintptr_t)pub, us, n,
                             (const void *)(uintptr_t)out);
    if (got != want) {
        char b[256];
        snprintf(b, sizeof b, "id %#x priv %#" PRIx64 "+%" PRIu64 " pub(%d) %#" PRIx64 "+%" PRIu64 " n %u out %#" PRIx64
                 ": got %#x want %#x", dh_id, priv, ps, (int)has_pub, pub, us, n, out, got, want);
        fail("check_dh", b);
    }
}

static void run_rules()
{
    const int ID = NOISE_DH_CURVE25519;
    const uint64_t strides[] = {0, 1, 31, 32, 33, 40, 64};
    const uint32_t counts[] = {0, 1, 2, 3};
    /* every small layout: the output walks across both inputs */
    for (uint32_t n : counts)
        for (uint64_t ps : strides)
            for (uint64_t us : strides)
                for (uint64_t out = 0x1000 - 140; out <= 0x1000 + 240; out += (out % 5 ? 3 : 1)) {
                    const uint64_t priv = 0x1000, pub = 0x1000 + 300;
                    expect(rules(ID, priv, ps, true, pub, us, n, out), ID, priv, ps, true, pub, us, n, out);
                    expect(rules(ID, priv, ps, true, out + 7, us, n, 0x1000 + 300), ID, priv, ps, true, out + 7, us, n,
                           0x1000 + 300);
                    expect(rules(ID, priv, ps, false, 0, 0, n, out), ID, priv, ps, false, 0, 0, n, out);
                }
    /* touching but not meeting, on both sides of each input, and one byte in */
    for (uint32_t n : {1u, 2u, 5u})
        for (uint64_t s : {0ull, 32ull, 40ull}) {
            const uint64_t in = 0x8000, span = (n - 1) * s + 32, far = 0x20000;
            expect(NOISE_ERROR_NONE, ID, in, s, true, far, 32, n, in + span);
            expect(NOISE_ERROR_INVALID_PARAM, ID, in, s, true, far, 32, n, in + span - 1);
            expect(NOISE_ERROR_NONE, ID, in, s, true, far, 32, n, in - 32 * n);
            expect(NOISE_ERROR_INVALID_PARAM, ID, in, s, true, far, 32, n, in - 32 * n + 1);
            expect(NOISE_ERROR_NONE, ID, far, 32, true, in, s, n, in + span);
            expect(NOISE_ERROR_INVALID_PARAM, ID, far, 32, true, in, s, n, in + span - 1);
            expect(NOISE_ERROR_NONE, ID, far, 32, true, in, s, n, in - 32 * n);
            expect(NOISE_ERROR_INVALID_PARAM, ID, far, 32, true, in, s, n, in - 32 * n + 1);
            expect(NOISE_ERROR_NONE, ID, in, s, false, 0, 0, n, in + span);
            expect(NOISE_ERROR_INVALID_PARAM, ID, in, s, false, 0, 0, n, in + span - 1);
            /* in place is refused too */
            expect(NOISE_ERROR_INVALID_PARAM, ID, in, s, true, far, 32, n, in);
            expect(NOISE_ERROR_INVALID_PARAM, ID, far, 32, true, in, s, n, in);
        }
    /* the order of the rules: the id first, then n == 0 before anything else */
    expect(NOISE_ERROR_UNKNOWN_ID, NOISE_ID('D', 2), 0x1000, 32, true, 0x2000, 32, 4, 0x3000);
    expect(NOISE_ERROR_UNKNOWN_ID, 0, 0, 5, true, 0, 5, 0, 0);
    expect(NOISE_ERROR_UNKNOWN_ID, NOISE_HASH_BLAKE2s, 0x1000, 32, false, 0, 0, 1, 0x3000);
    expect(NOISE_ERROR_NONE, ID, 0, 5, true, 0, 7, 0, 0);
    expect(NOISE_ERROR_NONE, ID, 0, 5, false, 0, 0, 0, 0);
    expect(NOISE_ERROR_INVALID_PARAM, ID, 0, 32, true, 0x2000, 32, 1, 0x3000);
    expect(NOISE_ERROR_INVALID_PARAM, ID, 0x1000, 32, true, 0, 32, 1, 0x3000);
    expect(NOISE_ERROR_INVALID_PARAM, ID, 0x1000, 32, true, 0x2000, 32, 1, 0);
    expect(NOISE_ERROR_INVALID_PARAM, ID, 0x1000, 32, false, 0, 0, 1, 0);
    expect(NOISE_ERROR_NONE, ID, 0x1000, 32, false, 0, 17, 1, 0x3000); /* no public value: its stride is not read */
    /* the edges of the arithmetic: nothing wraps */
    const uint32_t NMAX = 0xffffffffu;
    const uint64_t TOP = ~0ull;
    expect(NOISE_ERROR_NONE, ID, 0x1000, 0, true, 0x2000, 0, NMAX, 0x3000);
    expect(NOISE_ERROR_INVALID_PARAM, ID, 0x1000, 32, true, 0x2000, 0, NMAX, 0x3000);       /* priv runs over it */
    expect(NOISE_ERROR_INVALID_PARAM, ID, 0x1000, TOP, true, 0x800, 0, 2, 0x3000);          /* 2^64 + 0x1000 - 1 + 32 */
    expect(NOISE_ERROR_NONE, ID, 0x4000, TOP, true, 0x800, 0, 2, 0x3000);                   /* starts above it */
    expect(NOISE_ERROR_NONE, ID, TOP - 31, 0, true, 0x800, 0, 1, 0x3000);
    expect(NOISE_ERROR_INVALID_PARAM, ID, 0x800, 0, true, 0x100, 1ull << 63, 3, TOP - 63);  /* 0x100 + 2^64 + 32 */
    expect(NOISE_ERROR_NONE, ID, 0x800, 0, true, 0x100, 1ull << 63, 2, TOP - 63);
    expect(NOISE_ERROR_INVALID_PARAM, ID, 0x800, 0, true, TOP - 80, 0, 2, TOP - 63);
    expect(NOISE_ERROR_NONE, ID, 0x800, 0, true, TOP - 95, 0, 2, TOP - 63);                 /* ends where it starts */
    expect(NOISE_ERROR_INVALID_PARAM, ID, 8, 0, true, 64, 0, NMAX, 40);                     /* 32 n bytes from 40 */
    expect(NOISE_ERROR_NONE, ID, 8, 0, true, 40, 0, NMAX, 72);
}

int main()
{
    const long cases = run_cases();
    run_rules();
    printf("dh_check f25: %ld vectors %ld failures\n", g_f25, g_f25_failures);
    printf("dh_check: %ld cases %ld checks %ld failures\n", cases, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
