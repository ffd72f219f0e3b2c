/*
 * handshake_fallback_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd handshake_fallback_check;
 * tests/test_handshake_fallback_host.py).
 *
 * The host-only half of the Noise Pipes fallback (csrc/handshake_plan.h, its
 * last section; header section 15) on the CPU under ASan/UBSan.
 *
 *   stdout  for every prefix x cipher x hash a line
 *             fbname <psk> <cipher id> <hash id> <name> <length>
 *           then the plan of XXfallback as asan/handshake_check prints a
 *           pattern's, with the remote ephemeral among the keys:
 *             req XXfallback <I|R> <prefix> local_s=. local_e=. remote_s=. remote_e=. psk=.
 *             plan XXfallback <I|R> <prefix> <index> <W|R> keyed_in=. steps=... overhead=. next=...
 *           then the patterns a fallback may follow:
 *             from <pattern> <0|1>
 *           and the merge rule by the status in the fallback:
 *             merge <status> <take|keep|zero>
 *   argv    groups of `expect <status> <selected> <flags> <was initiator>
 *           <0|1>`: hs_fallback_takes, the function the kernel runs, must give
 *           the last word; a group that differs is reported "FAIL expect".
 *   then    the take-part rule over every status, select byte, flag word and
 *           role against the sentence of the header, and the argument checks
 *           of _fallback and _fallback_merge against a byte-by-byte reading of
 *           it: every small layout over never-dereferenced pointers.
 *
 * The last line: "handshake_fallback_check: <expectations> expectations
 * <checks> checks <failures> failures".
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

static const char *tok_name(HsTok t)
{
    static const char *names[] = {"e", "s", "ee", "es", "se", "ss"};
    return names[t];
}

static void print_names()
{
    for (int psk = 0; psk < 2; ++psk)
        for (int cipher : {NOISE_CIPHER_CHACHAPOLY, NOISE_CIPHER_AESGCM})
            for (int hash : {NOISE_HASH_BLAKE2s, NOISE_HASH_BLAKE2b, NOISE_HASH_SHA256, NOISE_HASH_SHA512}) {
                HsName n = {};
                n.pattern = 13;
                n.cipher_id = cipher;
                n.hash_id = hash;
                n.psk = psk;
                char name[HS_NAME_MAX];
                const size_t len = hs_fallback_name(n, name, sizeof(name));
                ++g_checks;
                if (!len || len != strlen(name) || len > 44) fail("name", name);
                /* a buffer one byte too small for the name and its NUL is refused, and not overrun */
                char *tight = (char *)malloc(len);
                ++g_checks;
                if (hs_fallback_name(n, tight, len) != 0) fail("tight name", name);
                free(tight);
                /* by name it stays out of reach */
                HsName parsed;
                ++g_checks;
                if (hs_parse_name(name, &parsed) != NOISE_ERROR_NOT_APPLICABLE) fail("parse", name);
                printf("fbname %d 0x%04x 0x%04x %s %zu\n", psk, cipher, hash, name, len);
            }
}

static void print_plan()
{
    const HsPattern &pat = HS_XXFALLBACK;
    for (int role : {NOISE_ROLE_INITIATOR, NOISE_ROLE_RESPONDER})
        for (int psk = 0; psk < 2; ++psk) {
            const bool init = hs_is_initiator(role);
            char who[64];
            snprintf(who, sizeof(who), "%s %c %s", pat.name, init ? 'I' : 'R', psk ? "NoisePSK" : "Noise");
            const HsNeeds need = hs_needs(pat, role);
            printf("req %s local_s=%d local_e=%d remote_s=%d remote_e=%d psk=%d\n", who, need.local_static,
                   need.local_ephemeral, need.remote_static, need.remote_ephemeral, psk);
            bool keyed = hs_keyed_before(pat, psk, 0); /* the pre-message e under NoisePSK */
            int action = hs_first_action(role);
            for (int idx = 0; idx < pat.n_msgs; ++idx) {
                ++g_checks;
                if (keyed != hs_keyed_before(pat, psk, idx)) fail("keyed", who);
                const HsMessage m = hs_message(pat, role, psk, idx, keyed);
                std::string steps;
                for (int t = 0; t < m.n_steps; ++t) {
                    const HsStep &s = m.steps[t];
                    if (t) steps += ",";
                    switch (s.kind) {
                    case HS_STEP_E: steps += s.mix_key ? "e+mk" : "e"; break;
                    case HS_STEP_S: steps += s.keyed ? "s+aead" : "s"; break;
                    case HS_STEP_DH:
                        steps += std::string(tok_name(s.tok)) + ":" + (s.priv_static ? "s" : "e") + "." +
                                 (s.pub_static ? "s" : "e");
                        break;
                    case HS_STEP_PAYLOAD: steps += s.keyed ? "p+aead" : "p"; break;
                    }
                }
                const bool writes = action == NOISE_ACTION_WRITE_MESSAGE;
                const char *next = m.next_action == NOISE_ACTION_SPLIT
                                       ? "split"
                                       : (m.next_action == NOISE_ACTION_WRITE_MESSAGE ? "write" : "read");
                printf("plan %s %d %c keyed_in=%d steps=%s overhead=%u next=%s\n", who, idx, writes ? 'W' : 'R', keyed,
                       steps.c_str(), m.overhead, next);
                keyed = m.keyed_after;
                action = m.next_action;
            }
            ++g_checks;
            if (action != NOISE_ACTION_SPLIT) fail("last action", who);
        }
    for (int p = 0; p < HS_N_PATTERNS; ++p) {
        printf("from %s %d\n", HS_PATTERNS[p].name, hs_fallback_possible(HS_PATTERNS[p]));
        /* the new field is the fallback's alone, and no row of the table is the fallback */
        ++g_checks;
        if (HS_PATTERNS[p].pre_r_e || !strcmp(HS_PATTERNS[p].name, HS_XXFALLBACK.name)) fail("table", HS_PATTERNS[p].name);
    }
    for (int st = 0; st < 256; ++st) {
        const HsMerge r = hs_fallback_merge_rule((uint8_t)st);
        if (st < 8 || st == 255) printf("merge %d %s\n", st, r == HS_MERGE_TAKE ? "take" : (r == HS_MERGE_KEEP ? "keep" : "zero"));
        ++g_checks;
        if (r != (st == 0 ? HS_MERGE_TAKE : (st == 5 ? HS_MERGE_KEEP : HS_MERGE_ZERO))) fail("merge", std::to_string(st));
    }
}

/* ---- the take-part rule, as the header words it */

static bool takes_rule(int status, int select_byte, bool have_select, uint32_t flags, bool was_initiator)
{
    const bool eligible = was_initiator ? status == 0 : (status == 0 || status == 1);
    if (!eligible) return false;
    if (have_select && select_byte == 0) return false;
    if ((flags & 1u) && status != 1) return false;
    return true;
}

static void check_takes()
{
    for (int status = 0; status < 256; ++status)
        for (int have_select = 0; have_select < 2; ++have_select)
            for (int byte : {0, 1, 2, 255})
                for (uint32_t flags = 0; flags < 2; ++flags)
                    for (int init = 0; init < 2; ++init) {
                        const bool selected = !have_select || byte != 0; /* as the kernel forms it */
                        ++g_checks;
                        if (hs_fallback_takes((uint8_t)status, selected, flags, init) !=
                            takes_rule(status, byte, have_select, flags, init)) {
                            char d[96];
                            snprintf(d, sizeof(d), "status=%d select=%d/%d flags=%u init=%d", status, have_select, byte, flags, init);
                            fail("takes", d);
                        }
                        /* who takes part was eligible */
                        ++g_checks;
                        if (hs_fallback_takes((uint8_t)status, selected, flags, init) &&
                            !hs_fallback_eligible((uint8_t)status, init))
                            fail("eligible", std::to_string(status));
                    }
}

static void check_expectations(int argc, char **argv)
{
    int i = 1;
    for (; i + 5 < argc && !strcmp(argv[i], "expect"); i += 6) {
        const bool got = hs_fallback_takes((uint8_t)atoi(argv[i + 1]), atoi(argv[i + 2]) != 0, (uint32_t)atoi(argv[i + 3]),
                                           atoi(argv[i + 4]) != 0);
        ++g_expect;
        if (got != (atoi(argv[i + 5]) != 0))
            fail("expect", std::string(argv[i + 1]) + " " + argv[i + 2] + " " + argv[i + 3] + " " + argv[i + 4]);
    }
    if (i != argc) fail("argument", argv[i]);
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
static const uint8_t *bptr(uint64_t v) { return (const uint8_t *)(uintptr_t)v; }

static void check_fallback_args()
{
    const int actions[] = {NOISE_ACTION_WRITE_MESSAGE, NOISE_ACTION_READ_MESSAGE, NOISE_ACTION_SPLIT, NOISE_ACTION_COMPLETE};
    const HsPattern *patterns[HS_N_PATTERNS + 2];
    for (int p = 0; p < HS_N_PATTERNS; ++p) patterns[p] = &HS_PATTERNS[p];
    patterns[HS_N_PATTERNS] = &HS_XXFALLBACK;
    patterns[HS_N_PATTERNS + 1] = nullptr; /* hs == NULL */
    for (const HsPattern *pat : patterns)
        for (int role : {NOISE_ROLE_INITIATOR, NOISE_ROLE_RESPONDER})
            for (int action : actions)
                for (int index = 0; index < 3; ++index)
                    for (int bits = 0; bits < 256; ++bits)
                        for (uint64_t stride : {0ull, 31ull, 32ull, 100ull}) {
                            const bool psk = bits & 1, has_static = bits & 2, give_e = bits & 4, give_psk = bits & 8;
                            const bool give_cfg = bits & 16, give_fb = bits & 32, give_prologue = bits & 64;
                            const uint32_t flags = (bits & 128) ? 3 : 1;
                            NoiseAeadHandshakeFallbackConfig cfg = {};
                            cfg.d_prologue = give_prologue ? bptr(64) : nullptr;
                            cfg.prologue_len = 32; /* a stride of 31 is below it */
                            cfg.prologue_stride = stride;
                            const uint64_t key_stride = stride == 100 ? 16 : stride; /* 100: only the key strides are short */
                            cfg.d_psk = give_psk ? bptr(4096) : nullptr;
                            cfg.psk_stride = key_stride;
                            cfg.d_local_ephemeral_priv = give_e ? bptr(8192) : nullptr;
                            cfg.local_ephemeral_stride = key_stride;
                            cfg.d_select = bptr(1);
                            cfg.flags = flags;
                            const bool init = role == NOISE_ROLE_INITIATOR;
                            /* the header's list, in its order */
                            int want = NOISE_ERROR_NONE;
                            const bool from_k = pat && pat != &HS_XXFALLBACK &&
                                                (!strcmp(pat->name, "NK") || !strcmp(pat->name, "XK") ||
                                                 !strcmp(pat->name, "KK") || !strcmp(pat->name, "IK"));
                            if (!pat || !give_cfg || !give_fb) want = NOISE_ERROR_INVALID_PARAM;
                            else if (!from_k) want = NOISE_ERROR_NOT_APPLICABLE;
                            else if (index != 1 || action != (init ? NOISE_ACTION_READ_MESSAGE : NOISE_ACTION_WRITE_MESSAGE))
                                want = NOISE_ERROR_INVALID_STATE;
                            else if (!has_static || (!init && !give_e)) want = NOISE_ERROR_LOCAL_KEY_REQUIRED;
                            else if (psk && !give_psk) want = NOISE_ERROR_PSK_REQUIRED;
                            else if (!give_prologue || stride == 31) want = NOISE_ERROR_INVALID_PARAM;
                            else if (stride == 100 && (psk || !init)) want = NOISE_ERROR_INVALID_PARAM; /* the keys that are read */
                            else if (flags & ~1u) want = NOISE_ERROR_INVALID_PARAM;
                            const HsFallbackFrom from = {pat, psk, role, action, index, has_static};
                            const int got = hs_check_fallback(from, give_cfg ? &cfg : nullptr, give_fb ? ptr(16) : nullptr);
                            ++g_checks;
                            if (got != want) {
                                char d[200];
                                snprintf(d, sizeof(d), "%s role=%#x action=%#x index=%d bits=%#x stride=%" PRIu64 ": got %#x want %#x",
                                         pat ? pat->name : "(null)", role, action, index, bits, stride, got, want);
                                fail("fallback check", d);
                            }
                        }
    /* an empty prologue needs no pointer, and a former initiator no key in cfg */
    NoiseAeadHandshakeFallbackConfig cfg = {};
    const HsFallbackFrom ik_i = {&HS_PATTERNS[13], false, NOISE_ROLE_INITIATOR, NOISE_ACTION_READ_MESSAGE, 1, true};
    ++g_checks;
    if (strcmp(HS_PATTERNS[13].name, "IK") || hs_check_fallback(ik_i, &cfg, ptr(16)) != NOISE_ERROR_NONE) fail("fallback check", "empty cfg");
}

static void check_merge_args()
{
    const int actions[] = {NOISE_ACTION_SPLIT, NOISE_ACTION_COMPLETE};
    const uint64_t FB_ST = 1000; /* the fallback's own statuses */
    const uint64_t places[] = {0, 2000, 2016, 2032, 2064, 2100, 2128, 3000, 3001, 999, 1001};
    for (int action : actions)
        for (uint32_t n = 0; n < 3; ++n)
            for (uint32_t hl : {32u, 64u})
                for (int null_at = -1; null_at < 9; ++null_at)
                    for (uint64_t moved : places)
                        for (int which = 0; which < 4; ++which) {
                            /* a layout with nothing meeting, then one output moved about */
                            uint64_t p[9] = {1 /* fb */, 5000 /* hs_status */, 6000 /* k1 */, 6200 /* k2 */, 2000 /* fb_k1 */,
                                             2064 /* fb_k2 */, 6400 /* h */, 2128 /* fb_h */, 6600 /* status */};
                            const int outs[4] = {2, 3, 6, 8};
                            p[outs[which]] = moved;
                            if (null_at >= 0) p[null_at] = 0;
                            if (null_at == 6 && moved == 3001) p[7] = 0; /* d_h and d_fb_h both NULL */
                            int want = NOISE_ERROR_NONE;
                            if (!p[0] || !p[1] || !p[2] || !p[3] || !p[4] || !p[5] || !p[8] || (!p[6] != !p[7]))
                                want = NOISE_ERROR_INVALID_PARAM;
                            else if (action != NOISE_ACTION_COMPLETE) want = NOISE_ERROR_INVALID_STATE;
                            else if (n) {
                                const Bytes out[4] = {mark(p[2], 32ull * n), mark(p[3], 32ull * n), mark(p[6], (uint64_t)hl * n),
                                                      mark(p[8], n)};
                                const Bytes in[5] = {mark(p[4], 32ull * n), mark(p[5], 32ull * n), mark(p[7], (uint64_t)hl * n),
                                                     mark(p[1], n), mark(FB_ST, n)};
                                for (const Bytes &o : out)
                                    for (const Bytes &i : in)
                                        if (meets(o, i)) want = NOISE_ERROR_INVALID_PARAM;
                            }
                            const int got = hs_check_fallback_merge(ptr(p[0]), action, n, hl, ptr(FB_ST), ptr(p[1]), ptr(p[2]),
                                                                    ptr(p[3]), ptr(p[4]), ptr(p[5]), ptr(p[6]), ptr(p[7]), ptr(p[8]));
                            ++g_checks;
                            if (got != want) {
                                char d[200];
                                snprintf(d, sizeof(d), "action=%#x n=%u hl=%u null_at=%d moved=%" PRIu64 " which=%d: got %#x want %#x",
                                         action, n, hl, null_at, moved, which, got, want);
                                fail("merge check", d);
                            }
                        }
}

int main(int argc, char **argv)
{
    print_names();
    print_plan();
    check_expectations(argc, argv);
    check_takes();
    check_fallback_args();
    check_merge_args();
    printf("handshake_fallback_check: %ld expectations %ld checks %ld failures\n", g_expect, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
