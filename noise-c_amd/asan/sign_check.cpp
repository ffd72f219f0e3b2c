/*
 * sign_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd sign_check; tests/test_sign_host.py).
 *
 * The Ed25519 arithmetic the GPU kernels run (csrc/sc25519.h, csrc/ge25519.h
 * over csrc/fe25519.h) and the host checks of noise_aead_dev_sign_verify /
 * _sign_public / _sign (csrc/dispatch.h check_sign_*) on the CPU under
 * ASan/UBSan.  hasher.h is device code, so where a kernel hashes, the case
 * carries the SHA-512 digest, which the test takes from hashlib.
 *
 *   stdin   one case per line, hex fields; the answer is printed as one line
 *           "<op> <result>" for the test to compare:
 *             red512 <64 bytes>           -> the value mod L, 32 bytes
 *             red256 <32 bytes>           -> the value mod L
 *             muladd <a> <b> <c>          -> a b + c mod L (canonical operands)
 *             decode <public key>         -> "1 <encode(-A)>" or "0"
 *             base <scalar>               -> encode([k]B), k canonical
 *             verify <public key> <signature> <SHA-512(R || A || M)>
 *                                         -> "<status> <encode([S]B - [h]A)>",
 *                                            or "<status> -" where the lane
 *                                            refuses before the walk
 *             public <SHA-512(seed)>      -> the public key
 *             sign <SHA-512(seed)> <SHA-512(prefix || M)> <SHA-512(R || A || M)>
 *                                         -> R || S
 *   then    the argument rules of the three entry points against a
 *           byte-by-byte reading of the header, over never-dereferenced
 *           pointers.
 *
 * Output: the answers, then the last line
 * "sign_check: <cases> cases <checks> checks <failures> failures" (failures:
 * lines that could not be read, and rule mismatches).
 */
#include "../csrc/dispatch.h"
#include "../csrc/ge25519.h"

#include <cinttypes>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

using namespace na;
typedef std::vector<uint8_t> Bytes;

static long g_checks, g_failures;

static void fail(const char *what, const std::string &detail)
{
    if (++g_failures <= 20) fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

static bool unhex(const std::string &s, size_t bytes, Bytes &out)
{
    auto nib = [](char c) { return c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1); };
    if (s.size() != 2 * bytes) return false;
    out.resize(bytes);
    for (size_t i = 0; i < bytes; ++i) {
        const int h = nib(s[2 * i]), l = nib(s[2 * i + 1]);
        if (h < 0 || l < 0) return false;
        out[i] = (uint8_t)(h * 16 + l);
    }
    return true;
}

static std::string hex(const Bytes &b)
{
    std::string s;
    char t[3];
    for (uint8_t x : b) {
        snprintf(t, sizeof t, "%02x", x);
        s += t;
    }
    return s;
}

/* results go through heap buffers of the exact size, so that ASan sees any
   access outside them */
static Bytes sc_bytes(const Sc &a)
{
    Bytes out(32, 0xA5);
    sc_store(out.data(), a);
    return out;
}

static Bytes f25_bytes(const F25 &a)
{
    Bytes out(32, 0xA5);
    f25_store(out.data(), a);
    return out;
}

/* what the kernels do with a seed's digest: ed25519_extsk, then mod L */
static Sc secret_scalar(Bytes digest)
{
    digest[0] &= 248;
    digest[31] &= 127;
    digest[31] |= 64;
    const Bytes low(digest.begin(), digest.begin() + 32);
    return sc_from_bytes32(low.data());
}

/* one lane of ed25519_verify_batch after the status test, the hash supplied */
static std::string lane_verify(const Bytes &pub, const Bytes &sig, const Bytes &hram)
{
    Ge na_;
    if ((sig[63] & 0xE0) || !ge_decode_negative(na_, pub.data())) return "6 -";
    const Sc h = sc_from_bytes64(hram.data());
    const Bytes sbytes(sig.begin() + 32, sig.end());
    const Sc s = sc_from_bytes32(sbytes.data());
    const F25 check = ge_encode(ge_double_scalarmult(s, h, na_));
    const Bytes rbytes(sig.begin(), sig.begin() + 32);
    const F25 r = f25_load(rbytes.data());
    uint32_t diff = 0;
    for (int j = 0; j < 8; ++j) diff |= check.v[j] ^ r.v[j];
    return std::string(diff ? "6 " : "0 ") + hex(f25_bytes(check));
}

static long run_cases()
{
    long cases = 0;
    char buf[4096];
    while (fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string op, f[3];
        in >> op >> f[0] >> f[1] >> f[2];
        if (op.empty()) continue;
        Bytes a, b, c;
        std::string out;
        if (op == "red512" && unhex(f[0], 64, a))
            out = hex(sc_bytes(sc_from_bytes64(a.data())));
        else if (op == "red256" && unhex(f[0], 32, a))
            out = hex(sc_bytes(sc_from_bytes32(a.data())));
        else if (op == "muladd" && unhex(f[0], 32, a) && unhex(f[1], 32, b) && unhex(f[2], 32, c)) {
            const F25 x = f25_load(a.data()), y = f25_load(b.data()), z = f25_load(c.data());
            Sc sa, sb, sc;
            for (int i = 0; i < 8; ++i) {
                sa.v[i] = x.v[i];
                sb.v[i] = y.v[i];
                sc.v[i] = z.v[i];
            }
            out = hex(sc_bytes(sc_muladd(sa, sb, sc)));
        } else if (op == "decode" && unhex(f[0], 32, a)) {
            Ge p;
            out = ge_decode_negative(p, a.data()) ? "1 " + hex(f25_bytes(ge_encode(p))) : "0";
        } else if (op == "base" && unhex(f[0], 32, a)) {
            const F25 x = f25_load(a.data());
            Sc k;
            for (int i = 0; i < 8; ++i) k.v[i] = x.v[i];
            out = hex(f25_bytes(ge_encode(ge_scalarmult_base(k))));
        } else if (op == "verify" && unhex(f[0], 32, a) && unhex(f[1], 64, b) && unhex(f[2], 64, c))
            out = lane_verify(a, b, c);
        else if (op == "public" && unhex(f[0], 64, a))
            out = hex(f25_bytes(ge_encode(ge_scalarmult_base(secret_scalar(a)))));
        else if (op == "sign" && unhex(f[0], 64, a) && unhex(f[1], 64, b) && unhex(f[2], 64, c)) {
            const Sc k = secret_scalar(a), r = sc_from_bytes64(b.data()), h = sc_from_bytes64(c.data());
            out = hex(f25_bytes(ge_encode(ge_scalarmult_base(r)))) + hex(sc_bytes(sc_muladd(h, k, r)));
        } else {
            fail("input", buf);
            continue;
        }
        ++cases;
        printf("%s %s\n", op.c_str(), out.c_str());
    }
    return cases;
}

/* ---- the argument rules, restated byte by byte */

struct Range { u128 ptr, stride; uint32_t item; bool present; };

static bool byte_in(u128 x, const Range &r, uint32_t n)
{
    if (!r.present) return false;
    u128 end = r.ptr + r.item; /* [ptr, ptr + (n - 1) stride + item) */
    if (n <= 64)
        for (uint32_t i = 1; i < n; ++i) end += r.stride;
    else
        end += (u128)(n - 1) * r.stride;
    return x >= r.ptr && x < end;
}

/* does any byte of the output [out, out + item n) lie in one of the ranges?
   Walks the bytes for small outputs and falls back to the ends for huge n. */
static bool output_meets(uint64_t out, uint32_t item, uint32_t n, const std::vector<Range> &ins)
{
    const u128 lo = out, hi = (u128)out + (u128)item * n;
    if (hi - lo <= 4096) {
        for (u128 x = lo; x < hi; ++x)
            for (const Range &r : ins)
                if (byte_in(x, r, n)) return true;
        return false;
    }
    for (const Range &r : ins) {
        if (!r.present) continue;
        const u128 rhi = r.ptr + (u128)(n - 1) * r.stride + r.item;
        if (lo < rhi && r.ptr < hi) return true;
    }
    return false;
}

struct V { int id; uint64_t pub, ps, sig, ss, msg, off, len; uint32_t n; uint64_t st_in, st; };

static int rules_verify(const V &v)
{
    if (v.id != NOISE_SIGN_ED25519) return NOISE_ERROR_UNKNOWN_ID;
    if (v.n == 0) return NOISE_ERROR_NONE;
    if (!v.pub || !v.sig || !v.msg || !v.off || !v.len || !v.st) return NOISE_ERROR_INVALID_PARAM;
    if (v.ps >= 1 && v.ps <= 31) return NOISE_ERROR_INVALID_PARAM;
    if (v.ss >= 1 && v.ss <= 63) return NOISE_ERROR_INVALID_PARAM;
    if (v.ss == 0 && v.n > 1) return NOISE_ERROR_INVALID_PARAM;
    std::vector<Range> ins = {{v.pub, v.ps, 32, true}, {v.sig, v.ss, 64, true}, {v.off, 8, 8, true},
                              {v.len, 4, 4, true}, {v.st_in, 1, 1, v.st_in != 0 && v.st_in != v.st}};
    return output_meets(v.st, 1, v.n, ins) ? NOISE_ERROR_INVALID_PARAM : NOISE_ERROR_NONE;
}

static void expect_verify(int want, const V &v)
{
    ++g_checks;
    auto p = [](uint64_t x) { return (const void *)(uintptr_t)x; };
    const int got = check_sign_verify(v.id, p(v.pub), v.ps, p(v.sig), v.ss, p(v.msg), p(v.off), p(v.len), v.n,
                                      p(v.st_in), p(v.st));
    if (got != want) {
        char b[320];
        snprintf(b, sizeof b, "id %#x pub %#" PRIx64 "+%" PRIu64 " sig %#" PRIx64 "+%" PRIu64 " msg %#" PRIx64
                 " off %#" PRIx64 " len %#" PRIx64 " n %u in %#" PRIx64 " out %#" PRIx64 ": got %#x want %#x",
                 v.id, v.pub, v.ps, v.sig, v.ss, v.msg, v.off, v.len, v.n, v.st_in, v.st, got, want);
        fail("check_sign_verify", b);
    }
}

struct S { int id; uint64_t priv, ps, pub, us, msg, off, len; uint32_t n; uint64_t out; };

static int rules_sign(const S &s)
{
    if (s.id != NOISE_SIGN_ED25519) return NOISE_ERROR_UNKNOWN_ID;
    if (s.n == 0) return NOISE_ERROR_NONE;
    if (!s.priv || !s.pub || !s.msg || !s.off || !s.len || !s.out) return NOISE_ERROR_INVALID_PARAM;
    if ((s.ps >= 1 && s.ps <= 31) || (s.us >= 1 && s.us <= 31)) return NOISE_ERROR_INVALID_PARAM;
    std::vector<Range> ins = {{s.priv, s.ps, 32, true}, {s.pub, s.us, 32, true}, {s.off, 8, 8, true},
                              {s.len, 4, 4, true}};
    return output_meets(s.out, 64, s.n, ins) ? NOISE_ERROR_INVALID_PARAM : NOISE_ERROR_NONE;
}

static void expect_sign(int want, const S &s)
{
    ++g_checks;
    auto p = [](uint64_t x) { return (const void *)(uintptr_t)x; };
    const int got = check_sign(s.id, p(s.priv), s.ps, p(s.pub), s.us, p(s.msg), p(s.off), p(s.len), s.n, p(s.out));
    if (got != want) {
        char b[320];
        snprintf(b, sizeof b, "id %#x priv %#" PRIx64 "+%" PRIu64 " pub %#" PRIx64 "+%" PRIu64 " msg %#" PRIx64
                 " off %#" PRIx64 " len %#" PRIx64 " n %u out %#" PRIx64 ": got %#x want %#x",
                 s.id, s.priv, s.ps, s.pub, s.us, s.msg, s.off, s.len, s.n, s.out, got, want);
        fail("check_sign", b);
    }
}

static int rules_public(int id, uint64_t priv, uint64_t ps, uint32_t n, uint64_t out)
{
    if (id != NOISE_SIGN_ED25519) return NOISE_ERROR_UNKNOWN_ID;
    if (n == 0) return NOISE_ERROR_NONE;
    if (!priv || !out) return NOISE_ERROR_INVALID_PARAM;
    if (ps >= 1 && ps <= 31) return NOISE_ERROR_INVALID_PARAM;
    return output_meets(out, 32, n, {{priv, ps, 32, true}}) ? NOISE_ERROR_INVALID_PARAM : NOISE_ERROR_NONE;
}

static void expect_public(int want, int id, uint64_t priv, uint64_t ps, uint32_t n, uint64_t out)
{
    ++g_checks;
    const int got = check_sign_public(id, (const void *)(uintptr_t)priv, ps, n, (const void *)(uintptr_t)out);
    if (got != want) {
        char b[200];
        snprintf(b, sizeof b, "id %#x priv %#" PRIx64 "+%" PRIu64 " n %u out %#" PRIx64 ": got %#x want %#x", id, priv,
                 ps, n, out, got, want);
        fail("check_sign_public", b);
    }
}

static void run_rules()
{
    const int ID = NOISE_SIGN_ED25519, BAD = NOISE_ERROR_INVALID_PARAM, OK = NOISE_ERROR_NONE;
    const uint64_t key_strides[] = {0, 1, 31, 32, 33, 40};
    const uint64_t sig_strides[] = {0, 1, 63, 64, 65, 72};
    const uint32_t counts[] = {0, 1, 2, 3};
    /* every small layout: the output walks across each input in turn, the
       inputs 0x400 apart */
    const V v0 = {ID, 0x1000, 32, 0x1400, 64, 0x1800, 0x1c00, 0x2000, 2, 0x2400, 0x2800};
    const S s0 = {ID, 0x1000, 32, 0x1400, 32, 0x1800, 0x1c00, 0x2000, 2, 0x2800};
    for (uint32_t n : counts)
        for (uint64_t ks : key_strides)
            for (uint64_t ss : sig_strides)
                for (uint64_t base : {0x1000ull, 0x1400ull, 0x1c00ull, 0x2000ull, 0x2400ull})
                    for (uint64_t d = 0; d <= 400; d += (d % 5 ? 3 : 1)) {
                        const uint64_t out = base - 200 + d;
                        V v = v0;
                        v.ps = ks, v.ss = ss, v.n = n, v.st = out;
                        expect_verify(rules_verify(v), v);
                        v.st_in = 0;
                        expect_verify(rules_verify(v), v);
                        S s = s0;
                        s.ps = ks, s.us = ss == 72 ? 40 : ks, s.n = n, s.out = out;
                        expect_sign(rules_sign(s), s);
                        if (base == 0x1000) expect_public(rules_public(ID, 0x1000, ks, n, out), ID, 0x1000, ks, n, out);
                    }
    /* the message buffer is not the host's to check: an output inside it passes */
    {
        V v = v0;
        v.st = v.msg;
        expect_verify(OK, v);
        S s = s0;
        s.out = s.msg;
        expect_sign(OK, s);
    }
    /* in place is the one overlap allowed; one byte off is not */
    for (uint32_t n : {1u, 2u, 64u}) {
        V v = v0;
        v.n = n, v.st = v.st_in;
        expect_verify(OK, v);
        v.st = v.st_in + 1;
        expect_verify(n > 1 ? BAD : OK, v);
        v.st = v.st_in - 1;
        expect_verify(n > 1 ? BAD : OK, v);
        v.st = v.st_in + n; /* touching */
        expect_verify(OK, v);
    }
    /* touching but not meeting, and one byte in, on both sides */
    for (uint32_t n : {1u, 2u, 5u})
        for (uint64_t s : {0ull, 32ull, 40ull}) {
            V v = v0;
            v.n = n, v.ps = s, v.ss = n > 1 ? 64 : 0;
            const uint64_t span = (n - 1) * s + 32, sspan = (n - 1) * v.ss + 64;
            v.st = v.pub + span;
            expect_verify(OK, v);
            v.st = v.pub + span - 1;
            expect_verify(BAD, v);
            v.st = v.pub - n;
            expect_verify(OK, v);
            v.st = v.pub - n + 1;
            expect_verify(BAD, v);
            v.st = v.sig + sspan;
            expect_verify(OK, v);
            v.st = v.sig + sspan - 1;
            expect_verify(BAD, v);
            v.st = v.off + 8 * n - 1;
            expect_verify(BAD, v);
            v.st = v.off + 8 * n;
            expect_verify(OK, v);
            v.st = v.len + 4 * n - 1;
            expect_verify(BAD, v);
            v.st = v.len + 4 * n;
            expect_verify(OK, v);
            S g = s0;
            g.n = n, g.ps = s, g.us = s;
            g.out = g.priv + span;
            expect_sign(OK, g);
            g.out = g.priv + span - 1;
            expect_sign(BAD, g);
            g.out = g.pub - 64 * n;
            expect_sign(OK, g);
            g.out = g.pub - 64 * n + 1;
            expect_sign(BAD, g);
            g.out = g.len + 4 * n - 1;
            expect_sign(BAD, g);
            expect_public(OK, ID, 0x8000, s, n, 0x8000 + span);
            expect_public(BAD, ID, 0x8000, s, n, 0x8000 + span - 1);
            expect_public(OK, ID, 0x8000, s, n, 0x8000 - 32 * n);
            expect_public(BAD, ID, 0x8000, s, n, 0x8000 - 32 * n + 1);
            expect_public(BAD, ID, 0x8000, s, n, 0x8000); /* in place is refused */
        }
    /* the order of the rules: the id first, then n == 0 before anything else,
       the pointers before the strides */
    {
        V v = v0;
        v.id = NOISE_ID('S', 2);
        expect_verify(NOISE_ERROR_UNKNOWN_ID, v);
        v.n = 0, v.pub = 0;
        expect_verify(NOISE_ERROR_UNKNOWN_ID, v);
        v = V{ID, 0, 5, 0, 7, 0, 0, 0, 0, 0, 0};
        expect_verify(OK, v);
        for (int k = 0; k < 6; ++k) {
            v = v0;
            (k == 0 ? v.pub : k == 1 ? v.sig : k == 2 ? v.msg : k == 3 ? v.off : k == 4 ? v.len : v.st) = 0;
            expect_verify(BAD, v);
        }
        v = v0;
        v.st_in = 0;
        expect_verify(OK, v);
        v = v0;
        v.n = 1, v.ss = 0;
        expect_verify(OK, v);
        v.n = 2;
        expect_verify(BAD, v);
        S s = s0;
        s.id = NOISE_DH_CURVE25519;
        expect_sign(NOISE_ERROR_UNKNOWN_ID, s);
        s = S{ID, 0, 5, 0, 7, 0, 0, 0, 0, 0};
        expect_sign(OK, s);
        for (int k = 0; k < 6; ++k) {
            s = s0;
            (k == 0 ? s.priv : k == 1 ? s.pub : k == 2 ? s.msg : k == 3 ? s.off : k == 4 ? s.len : s.out) = 0;
            expect_sign(BAD, s);
        }
        expect_public(NOISE_ERROR_UNKNOWN_ID, 0, 0x1000, 32, 4, 0x3000);
        expect_public(NOISE_ERROR_UNKNOWN_ID, NOISE_ID('S', 2), 0, 5, 0, 0);
        expect_public(OK, ID, 0, 5, 0, 0);
        expect_public(BAD, ID, 0, 32, 1, 0x3000);
        expect_public(BAD, ID, 0x1000, 32, 1, 0);
    }
    /* the edges of the arithmetic: nothing wraps */
    const uint32_t NMAX = 0xffffffffu;
    const uint64_t TOP = ~0ull;
    expect_public(OK, ID, 0x1000, 0, NMAX, 0x3000);
    expect_public(BAD, ID, 0x3000, 32, NMAX, 0x1000);   /* 32 n bytes from 0x1000 run over it */
    expect_public(BAD, ID, 0x1000, TOP, 2, 0x3000);     /* the span ends at 2^64 + 0x1000 - 1 + 32 */
    expect_public(OK, ID, 0x4000, TOP, 2, 0x3000);      /* starts above it */
    expect_public(OK, ID, TOP - 31, 0, 1, 0x3000);
    {
        V v = v0;
        v.n = NMAX, v.ps = 0, v.ss = 64, v.pub = 0x100, v.sig = 0x200, v.off = 0x10, v.len = 0x20, v.st_in = 0;
        v.st = 0x80; /* n bytes from 0x80 run over the key */
        expect_verify(BAD, v);
        v.ss = 1ull << 63, v.n = 3, v.sig = 0x100, v.pub = 0x40, v.st = TOP - 63; /* 0x100 + 2^64 + 64 */
        expect_verify(BAD, v);
        v.n = 2;
        expect_verify(OK, v);
    }
}

int main()
{
    const long cases = run_cases();
    run_rules();
    printf("sign_check: %ld cases %ld checks %ld failures\n", cases, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
