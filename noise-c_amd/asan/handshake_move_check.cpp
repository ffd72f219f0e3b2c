/*
 * handshake_move_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd handshake_move_check;
 * tests/test_handshake_move_host.py).
 *
 * The host-only half of the sessions that change their object
 * (csrc/handshake_plan.h, its last section; header section 16) on the CPU
 * under ASan/UBSan.
 *
 *   stdout  for every (in range, in range, status 0..5, status 0..5) a line
 *             rule <src in range> <dst in range> <src status> <dst status> <result>
 *           from hs_move_rule, the function the kernel runs; then, for two
 *           positions that differ in exactly one field,
 *             position <field> <0|1>
 *           and "position none 1" for two equal ones.
 *   argv    groups of `expect <src in range> <dst in range> <src status>
 *           <dst status> <result>`: hs_move_rule must give the last word; a
 *           group that differs is reported "FAIL expect".
 *   then    the rule over every status byte against the table of the header,
 *           and the argument checks of _new_like, _move and _drop against a
 *           byte-by-byte reading of it, in its order: every small layout over
 *           never-dereferenced pointers.
 *
 * The last line: "handshake_move_check: <expectations> expectations <checks>
 * checks <failures> failures".
 */
#include "../csrc/handshake_plan.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

using namespace na;

static long g_expect, g_checks, g_failures;

static void fail(const char *what, const std::string &detail)
{
    if (++g_failures <= 20) fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

/* ---- the rule of one entry, as the header's table words it */

static int rule_of_the_header(bool src_in, bool dst_in, int ss, int ds)
{
    if (!src_in) return 3; /* a lane number >= n of its object */
    if (!dst_in) return 3;
    if (ss == 5) return 1; /* the source lane is empty */
    if (ds != 5) return 2; /* the destination lane is not */
    return 0;
}

static void print_rule()
{
    for (int si = 0; si < 2; ++si)
        for (int di = 0; di < 2; ++di)
            for (int ss = 0; ss < 6; ++ss)
                for (int ds = 0; ds < 6; ++ds)
                    printf("rule %d %d %d %d %d\n", si, di, ss, ds, hs_move_rule(si, di, (uint8_t)ss, (uint8_t)ds));
    for (int si = 0; si < 2; ++si)
        for (int di = 0; di < 2; ++di)
            for (int ss = 0; ss < 256; ++ss)
                for (int ds = 0; ds < 256; ++ds) {
                    ++g_checks;
                    if (hs_move_rule(si, di, (uint8_t)ss, (uint8_t)ds) != rule_of_the_header(si, di, ss, ds))
                        fail("rule", std::to_string(si) + " " + std::to_string(di) + " " + std::to_string(ss) + " " +
                                         std::to_string(ds));
                }
    ++g_checks;
    if (NOISE_AEAD_MOVED != 0 || NOISE_AEAD_MOVE_EMPTY != 1 || NOISE_AEAD_MOVE_TAKEN != 2 || NOISE_AEAD_MOVE_RANGE != 3 ||
        HS_STATUS_ABSENT != 5)
        fail("constants", "");
}

static void check_expectations(int argc, char **argv)
{
    int i = 1;
    for (; i + 5 < argc && !strcmp(argv[i], "expect"); i += 6) {
        const int got = hs_move_rule(atoi(argv[i + 1]) != 0, atoi(argv[i + 2]) != 0, (uint8_t)atoi(argv[i + 3]),
                                     (uint8_t)atoi(argv[i + 4]));
        ++g_expect;
        if (got != atoi(argv[i + 5]))
            fail("expect", std::string(argv[i + 1]) + " " + argv[i + 2] + " " + argv[i + 3] + " " + argv[i + 4]);
    }
    if (i != argc) fail("argument", argv[i]);
}

/* ---- positions */

static HsPosition base_position()
{
    HsPosition p = {};
    p.name.pattern = 8;
    p.name.cipher_id = NOISE_CIPHER_CHACHAPOLY;
    p.name.hash_id = NOISE_HASH_BLAKE2s;
    p.name.psk = false;
    p.fallback = false;
    p.role = NOISE_ROLE_RESPONDER;
    p.action = NOISE_ACTION_READ_MESSAGE;
    p.index = 2;
    p.keyed = true;
    p.nonce = 1;
    return p;
}

static const char *FIELDS[] = {"pattern", "cipher", "hash", "psk", "fallback", "role", "action", "index", "keyed", "nonce"};
constexpr int N_FIELDS = 10;

/* the base position with one field changed (field < 0: none) */
static HsPosition changed(int field)
{
    HsPosition p = base_position();
    switch (field) {
    case 0: p.name.pattern = 7; break;
    case 1: p.name.cipher_id = NOISE_CIPHER_AESGCM; break;
    case 2: p.name.hash_id = NOISE_HASH_SHA256; break;
    case 3: p.name.psk = true; break;
    case 4: p.fallback = true; break;
    case 5: p.role = NOISE_ROLE_INITIATOR; break;
    case 6: p.action = NOISE_ACTION_WRITE_MESSAGE; break;
    case 7: p.index = 1; break;
    case 8: p.keyed = false; break;
    case 9: p.nonce = 1ull << 32 | 1; break; /* differs in its high half alone */
    default: break;
    }
    return p;
}

static void print_positions()
{
    const HsPosition base = base_position();
    for (int f = 0; f < N_FIELDS; ++f) {
        const bool same = hs_same_position(base, changed(f));
        ++g_checks;
        if (same != hs_same_position(changed(f), base)) fail("position symmetry", FIELDS[f]);
        ++g_checks;
        if (!hs_same_position(changed(f), changed(f))) fail("position reflexive", FIELDS[f]);
        printf("position %s %d\n", FIELDS[f], same);
    }
    printf("position none %d\n", hs_same_position(base, changed(-1)));
}

/* ---- the argument checks, byte by byte */

typedef std::set<uint64_t> Bytes;

static Bytes mark(uint64_t p, uint64_t len)
{
    Bytes b;
    if (p)
        for (uint64_t j = 0; j < len; ++j) b.insert(p + j);
    return b;
}

static bool meets(const Bytes &a, const Bytes &b)
{
    for (uint64_t x : a)
        if (b.count(x)) return true;
    return false;
}

static const void *ptr(uint64_t v) { return (const void *)(uintptr_t)v; }

static void check_new_like_args()
{
    const int actions[] = {NOISE_ACTION_NONE, NOISE_ACTION_WRITE_MESSAGE, NOISE_ACTION_READ_MESSAGE, NOISE_ACTION_FAILED,
                           NOISE_ACTION_SPLIT, NOISE_ACTION_COMPLETE};
    for (int action : actions)
        for (int give_out = 0; give_out < 2; ++give_out)
            for (int give_like = 0; give_like < 2; ++give_like) {
                int want = NOISE_ERROR_NONE;
                if (!give_out || !give_like) want = NOISE_ERROR_INVALID_PARAM;
                else if (action == NOISE_ACTION_COMPLETE || action == NOISE_ACTION_NONE || action == NOISE_ACTION_FAILED)
                    want = NOISE_ERROR_INVALID_STATE; /* no object of this library is ever at _FAILED */
                const int got = hs_check_new_like(give_out ? ptr(8) : nullptr, give_like ? ptr(16) : nullptr, action);
                ++g_checks;
                if (got != want) fail("new_like check", std::to_string(action) + " " + std::to_string(give_out) + std::to_string(give_like));
            }
}

/* how one object holds one key, by number: 0 none, 1 shared at pointer A, 2
   shared at pointer B, 3 per session in the caller's rows, 4 per session in
   owned rows */
static HsKey key_of(int kind)
{
    switch (kind) {
    case 1: return {HS_HOLD_SHARED, ptr(0x7000), false};
    case 2: return {HS_HOLD_SHARED, ptr(0x7020), false};
    case 3: return {HS_HOLD_EACH, ptr(0x8000), false};
    case 4: return {HS_HOLD_EACH, ptr(0x9000), true};
    default: return {HS_HOLD_NONE, nullptr, false};
    }
}

/* rule 4 for one key: dst's kind against src's */
static bool keys_agree(int dst, int src)
{
    if (dst == 0 || src == 0) return dst == src;           /* neither holds it */
    if (dst <= 2 || src <= 2) return dst == src;           /* once for all, through the same pointer */
    return dst == 4;                                       /* both per session, dst in rows it owns */
}

static void check_move_args()
{
    const int actions[] = {NOISE_ACTION_WRITE_MESSAGE, NOISE_ACTION_READ_MESSAGE, NOISE_ACTION_SPLIT, NOISE_ACTION_COMPLETE,
                           NOISE_ACTION_NONE};
    const uint64_t results[] = {0, 5000, 1999, 2000, 2011, 2012, 2999, 3000, 3003, 3004};
    long combos = 0;
    for (int objs = 0; objs < 5; ++objs)          /* 0 both, 1 no dst, 2 no src, 3 neither, 4 the same object */
        for (int field = -1; field < N_FIELDS; ++field)
            for (int action : actions)
                for (int dk = 0; dk < 5; ++dk)
                    for (int sk = 0; sk < 5; ++sk)
                        for (int ek = 0; ek < 2; ++ek)   /* the ephemeral key: agreeing, or not */
                            for (uint32_t m : {0u, 1u, 3u, 4u})
                                for (int lists = 0; lists < 4; ++lists)
                                    for (uint64_t res : results) {
                                        /* thin the product: the layouts of d_result only where the earlier rules pass */
                                        const bool early = objs || field >= 0 || !keys_agree(dk, sk) || ek;
                                        if (early && res != 0 && res != 2000) continue;
                                        ++combos;
                                        const uint32_t n_dst = 3, n_src = 3;
                                        const uint64_t dl = (lists & 1) ? 2000 : 0, sl = (lists & 2) ? 3000 : 0;
                                        HsMoveSide dst = {}, src = {};
                                        dst.obj = (objs == 1 || objs == 3) ? nullptr : ptr(64);
                                        src.obj = (objs == 2 || objs == 3) ? nullptr : (objs == 4 ? ptr(64) : ptr(128));
                                        dst.pos = changed(field);
                                        src.pos = base_position();
                                        src.pos.action = action;
                                        dst.pos.action = field != 6 ? action
                                                                    : (action == NOISE_ACTION_WRITE_MESSAGE ? NOISE_ACTION_READ_MESSAGE
                                                                                                            : NOISE_ACTION_WRITE_MESSAGE);
                                        dst.keys[0] = key_of(dk);
                                        src.keys[0] = key_of(sk);
                                        dst.keys[1] = key_of(ek ? 3 : 4);
                                        src.keys[1] = key_of(3);
                                        dst.n = n_dst;
                                        src.n = n_src;
                                        dst.d_lanes = ptr(dl);
                                        src.d_lanes = ptr(sl);
                                        /* the header's list, in its order */
                                        int want = NOISE_ERROR_NONE;
                                        const bool movable = action == NOISE_ACTION_WRITE_MESSAGE ||
                                                             action == NOISE_ACTION_READ_MESSAGE || action == NOISE_ACTION_SPLIT;
                                        if (!dst.obj || !src.obj) want = NOISE_ERROR_INVALID_PARAM;
                                        else if (dst.obj == src.obj) want = NOISE_ERROR_INVALID_PARAM;
                                        else if (field >= 0 || !movable) want = NOISE_ERROR_INVALID_STATE;
                                        else if (!keys_agree(dk, sk) || ek) want = NOISE_ERROR_INVALID_PARAM;
                                        else if (m == 0) want = NOISE_ERROR_NONE;
                                        else if ((!dl && m > n_dst) || (!sl && m > n_src)) want = NOISE_ERROR_INVALID_PARAM;
                                        else if (meets(mark(res, m), mark(dl, 4ull * m)) || meets(mark(res, m), mark(sl, 4ull * m)))
                                            want = NOISE_ERROR_INVALID_PARAM;
                                        const int got = hs_check_move(dst, src, m, ptr(res));
                                        ++g_checks;
                                        if (got != want) {
                                            char d[240];
                                            snprintf(d, sizeof(d), "objs=%d field=%d action=%#x keys=%d/%d/%d m=%u lists=%d result=%" PRIu64
                                                     ": got %#x want %#x", objs, field, action, dk, sk, ek, m, lists, res, got, want);
                                            fail("move check", d);
                                        }
                                    }
    ++g_checks;
    if (combos < 20000) fail("move check", "too few layouts");
}

static void check_drop_args()
{
    for (int give_hs = 0; give_hs < 2; ++give_hs)
        for (int give_lanes = 0; give_lanes < 2; ++give_lanes)
            for (uint32_t n : {0u, 1u, 5u})
                for (uint32_t m : {0u, 1u, 5u, 6u}) {
                    int want = NOISE_ERROR_NONE;
                    if (!give_hs) want = NOISE_ERROR_INVALID_PARAM;
                    else if (m == 0) want = NOISE_ERROR_NONE;
                    else if (m > n) want = NOISE_ERROR_INVALID_PARAM;
                    else if (!give_lanes) want = NOISE_ERROR_INVALID_PARAM;
                    const int got = hs_check_drop(give_hs ? ptr(64) : nullptr, n, give_lanes ? ptr(2000) : nullptr, m);
                    ++g_checks;
                    if (got != want) fail("drop check", std::to_string(give_hs) + std::to_string(give_lanes) + " " + std::to_string(n) + " " + std::to_string(m));
                }
}

/* _fallback of an object made by _new_like: refused where a fallback is refused, before the state and the keys */
static void check_fallback_of_made_like()
{
    NoiseAeadHandshakeFallbackConfig cfg = {};
    HsFallbackFrom ik = {&HS_PATTERNS[13], false, NOISE_ROLE_INITIATOR, NOISE_ACTION_READ_MESSAGE, 1, true};
    ++g_checks;
    if (strcmp(HS_PATTERNS[13].name, "IK") || ik.made_like || hs_check_fallback(ik, &cfg, ptr(16)) != NOISE_ERROR_NONE)
        fail("fallback", "an ordinary object");
    ik.made_like = true;
    ++g_checks;
    if (hs_check_fallback(ik, &cfg, ptr(16)) != NOISE_ERROR_NOT_APPLICABLE) fail("fallback", "made like");
    ik.index = 0; /* a wrong state as well: the first cause wins */
    ++g_checks;
    if (hs_check_fallback(ik, &cfg, ptr(16)) != NOISE_ERROR_NOT_APPLICABLE) fail("fallback", "made like, wrong state");
    ++g_checks;
    if (hs_check_fallback(ik, nullptr, ptr(16)) != NOISE_ERROR_INVALID_PARAM) fail("fallback", "made like, no cfg");
}

int main(int argc, char **argv)
{
    print_rule();
    print_positions();
    check_expectations(argc, argv);
    check_new_like_args();
    check_move_args();
    check_drop_args();
    check_fallback_of_made_like();
    printf("handshake_move_check: %ld expectations %ld checks %ld failures\n", g_expect, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
