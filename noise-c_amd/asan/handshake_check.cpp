/*
 * handshake_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd handshake_check; tests/test_handshake_host.py).
 *
 * The host-only half of the batched handshakes (csrc/handshake_plan.h) on the
 * CPU under ASan/UBSan.
 *
 *   stdout  for every pattern x role x prefix, a line
 *             req <pattern> <I|R> <prefix> local_s=. local_e=. remote_s=. psk=.
 *           and for each message a line
 *             plan <pattern> <I|R> <prefix> <index> <W|R> keyed_in=. steps=... overhead=. next=...
 *           a step being e / e+mk, s / s+aead, <dh>:<local>.<remote> (each
 *           side e or s), p / p+aead; the test compares them with the table
 *           of tests/handshake_model.py.
 *   stdin   one protocol name per line; each is answered with
 *             name <name> <rc as 0x....> [<pattern> <cipher id> <hash id> <psk>]
 *   then    the argument checks of write_message, read_message and split
 *           against a byte-by-byte reading of the header comment: every small
 *           layout (pointers, strides, lengths, counts) over never-dereferenced
 *           pointers, with the spans marked byte by byte, and layouts at the
 *           edges of 64-bit arithmetic.
 *
 * The last line: "handshake_check: <plans> plans <names> names <checks>
 * checks <failures> failures".
 */
#include "../csrc/handshake_plan.h"

#include <cinttypes>
#include <cstdio>
#include <set>
#include <string>

using namespace na;

static long g_plans, g_names, g_checks, g_failures;

static void fail(const char *what, const std::string &detail)
{
    if (++g_failures <= 20) fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

static const char *tok_name(HsTok t)
{
    static const char *names[] = {"e", "s", "ee", "es", "se", "ss"};
    return names[t];
}

static void print_plans()
{
    const int roles[2] = {NOISE_ROLE_INITIATOR, NOISE_ROLE_RESPONDER};
    for (int p = 0; p < HS_N_PATTERNS; ++p)
        for (int role : roles)
            for (int psk = 0; psk < 2; ++psk) {
                const HsPattern &pat = HS_PATTERNS[p];
                const bool init = hs_is_initiator(role);
                char who[64];
                snprintf(who, sizeof(who), "%s %c %s", pat.name, init ? 'I' : 'R', psk ? "NoisePSK" : "Noise");
                const HsNeeds need = hs_needs(pat, role);
                printf("req %s local_s=%d local_e=%d remote_s=%d psk=%d\n", who, need.local_static, need.local_ephemeral,
                       need.remote_static, psk);
                bool keyed = false;
                int action = hs_first_action(role);
                for (int idx = 0; idx < pat.n_msgs; ++idx) {
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
                    if (writes != ((idx % 2 == 0) == init)) fail("direction", who);
                    const char *next = m.next_action == NOISE_ACTION_SPLIT
                                           ? "split"
                                           : (m.next_action == NOISE_ACTION_WRITE_MESSAGE ? "write" : "read");
                    printf("plan %s %d %c keyed_in=%d steps=%s overhead=%u next=%s\n", who, idx, writes ? 'W' : 'R', keyed,
                           steps.c_str(), m.overhead, next);
                    keyed = m.keyed_after;
                    action = m.next_action;
                    ++g_plans;
                }
                if (action != NOISE_ACTION_SPLIT) fail("last action", who);
            }
}

static void answer_names()
{
    char line[512];
    while (fgets(line, sizeof(line), stdin)) {
        size_t n = strlen(line);
        while (n && (line[n - 1] == '\n' || line[n - 1] == '\r')) line[--n] = 0;
        HsName r;
        const int rc = hs_parse_name(line, &r);
        if (rc) printf("name %s 0x%04x\n", line, rc);
        else printf("name %s 0x%04x %s 0x%04x 0x%04x %d\n", line, rc, HS_PATTERNS[r.pattern].name, r.cipher_id, r.hash_id, r.psk);
        ++g_names;
    }
}

/* ---- the header's rules, byte by byte */

typedef std::set<uint64_t> Bytes;

static Bytes mark(uint64_t p, uint64_t stride, uint64_t len, uint32_t n)
{
    Bytes b;
    for (uint32_t i = 0; i < n; ++i)
        for (uint64_t j = 0; j < len; ++j) b.insert(p + i * stride + j);
    return b;
}

static bool meets(const Bytes &a, const Bytes &b)
{
    for (uint64_t x : a)
        if (b.count(x)) return true;
    return false;
}

static const void *ptr(uint64_t v) { return (const void *)(uintptr_t)v; }

static int read_write_rule(bool write, int action, uint32_t n, uint32_t overhead, uint64_t pp, uint64_t ps, uint32_t pl,
                           uint64_t mp, uint64_t ms, uint32_t ml)
{
    /* write: pl given, ml = pl + overhead; read: ml given, pl = ml - overhead */
    if (action != (write ? NOISE_ACTION_WRITE_MESSAGE : NOISE_ACTION_READ_MESSAGE)) return NOISE_ERROR_INVALID_STATE;
    if (write) {
        if ((uint64_t)pl + overhead > 65535) return NOISE_ERROR_INVALID_LENGTH;
        ml = pl + overhead;
    } else {
        if (ml > 65535 || ml < overhead) return NOISE_ERROR_INVALID_LENGTH;
        pl = ml - overhead;
    }
    if (!n) return NOISE_ERROR_NONE;
    if (!mp || (pl && !pp)) return NOISE_ERROR_INVALID_PARAM;
    /* the input may sit at stride 0 (one value for all) or at least its length; the output at least its length */
    const uint64_t in_stride = write ? ps : ms, out_stride = write ? ms : ps;
    const uint32_t in_len = write ? pl : ml, out_len = write ? ml : pl;
    if (in_len && in_stride && in_stride < in_len) return NOISE_ERROR_INVALID_PARAM;
    if (out_len && out_stride < out_len) return NOISE_ERROR_INVALID_PARAM;
    /* spans, not records: first byte of slot 0 to last byte of slot n - 1 */
    const uint64_t in_p = write ? pp : mp, out_p = write ? mp : pp;
    if (in_len && out_len) {
        const Bytes in = mark(in_p, 1, (n - 1) * in_stride + in_len, 1), out = mark(out_p, 1, (n - 1) * out_stride + out_len, 1);
        if (meets(in, out)) return NOISE_ERROR_INVALID_PARAM;
    }
    return NOISE_ERROR_NONE;
}

static void check_messages()
{
    const int actions[] = {NOISE_ACTION_WRITE_MESSAGE, NOISE_ACTION_READ_MESSAGE, NOISE_ACTION_SPLIT};
    const uint64_t strides[] = {0, 1, 2, 3, 5, 8};
    for (int write = 0; write < 2; ++write)
        for (int action : actions)
            for (uint32_t n = 0; n < 4; ++n)
                for (uint32_t overhead = 0; overhead < 3; ++overhead)
                    for (uint32_t len = 0; len < 4; ++len) /* write: payload_len; read: msg_len */
                        for (uint64_t ps : strides)
                            for (uint64_t ms : strides)
                                for (uint64_t pp : {0ull, 16ull, 20ull})
                                    for (uint64_t mp = 0; mp < 40; mp += (mp < 8 ? 8 : 1)) {
                                        const int want = read_write_rule(write, action, n, overhead, pp, ps, len, mp, ms, len);
                                        const int got =
                                            write ? hs_check_write(action, n, overhead, ptr(pp), ps, len, ptr(mp), ms)
                                                  : hs_check_read(action, n, overhead, ptr(mp), ms, len, ptr(pp), ps);
                                        ++g_checks;
                                        if (got != want) {
                                            char d[200];
                                            snprintf(d, sizeof(d),
                                                     "write=%d action=%#x n=%u over=%u len=%u pp=%" PRIu64 " ps=%" PRIu64
                                                     " mp=%" PRIu64 " ms=%" PRIu64 ": got %#x want %#x",
                                                     write, action, n, overhead, len, pp, ps, mp, ms, got, want);
                                            fail("message check", d);
                                        }
                                    }
    /* the lengths at their limits, and spans beyond 64 bits: a span of
       (n - 1) * stride + len bytes is computed without wrapping */
    struct Edge { int got, want; const char *what; };
    const uint64_t top = ~0ull;
    const Edge edges[] = {
        {hs_check_write(NOISE_ACTION_WRITE_MESSAGE, 2, 48, ptr(64), 0, 65535 - 48, ptr(1 << 20), 65535), 0, "longest write"},
        {hs_check_write(NOISE_ACTION_WRITE_MESSAGE, 2, 48, ptr(64), 0, 65535 - 47, ptr(1 << 20), 65536), NOISE_ERROR_INVALID_LENGTH, "write one over"},
        {hs_check_write(NOISE_ACTION_WRITE_MESSAGE, 2, 48, ptr(64), 0, 0xFFFFFFFFu, ptr(1 << 20), top), NOISE_ERROR_INVALID_LENGTH, "write 2^32 - 1"},
        {hs_check_read(NOISE_ACTION_READ_MESSAGE, 2, 48, ptr(64), 65535, 65535, ptr(1 << 20), 65535), 0, "longest read"},
        {hs_check_read(NOISE_ACTION_READ_MESSAGE, 2, 48, ptr(64), 65536, 65536, ptr(1 << 20), 65536), NOISE_ERROR_INVALID_LENGTH, "read one over"},
        {hs_check_read(NOISE_ACTION_READ_MESSAGE, 2, 48, ptr(64), 64, 47, ptr(1 << 20), 64), NOISE_ERROR_INVALID_LENGTH, "read below overhead"},
        {hs_check_read(NOISE_ACTION_READ_MESSAGE, 2, 48, ptr(64), 64, 48, nullptr, 0), 0, "read, empty payload, no pointer"},
        /* a message span that a 64-bit sum would wrap round to the low payload */
        {hs_check_write(NOISE_ACTION_WRITE_MESSAGE, 0xFFFFFFFFu, 32, ptr(8), 8, 8, ptr(top - 255), 1ull << 40), 0, "span past 2^64"},
        {hs_check_write(NOISE_ACTION_WRITE_MESSAGE, 0xFFFFFFFFu, 32, ptr(top - 100), 8, 8, ptr(64), 1ull << 40), NOISE_ERROR_INVALID_PARAM, "wide span meets a high payload"},
        {hs_check_read(NOISE_ACTION_READ_MESSAGE, 3, 32, ptr(top - 200), 0, 40, ptr(64), top / 2), NOISE_ERROR_INVALID_PARAM, "payload span over a high message"},
        {hs_check_read(NOISE_ACTION_READ_MESSAGE, 2, 32, ptr(top - 200), 0, 40, ptr(64), top / 2), 0, "payload span ends below a high message"},
    };
    for (const Edge &e : edges) {
        ++g_checks;
        if (e.got != e.want) fail("edge", e.what);
    }
}

static void check_splits()
{
    const int actions[] = {NOISE_ACTION_WRITE_MESSAGE, NOISE_ACTION_SPLIT, NOISE_ACTION_COMPLETE};
    for (int action : actions)
        for (uint32_t n = 0; n < 3; ++n)
            for (uint32_t hl : {32u, 64u})
                for (uint64_t k1 = 0; k1 <= 256; k1 += 32)
                    for (uint64_t k2 : {0ull, 1ull, 31ull, 32ull, 33ull, 63ull, 64ull, 65ull, 95ull, 96ull, 127ull, 128ull, 160ull, 191ull, 192ull, 300ull})
                        for (uint64_t hh : {0ull, 100ull, 129ull, 400ull}) {
                            int want;
                            if (action != NOISE_ACTION_SPLIT) want = NOISE_ERROR_INVALID_STATE;
                            else if (!n) want = NOISE_ERROR_NONE;
                            else if (!k1 || !k2) want = NOISE_ERROR_INVALID_PARAM;
                            else {
                                const Bytes a = mark(k1, 0, 32ull * n, 1), b = mark(k2, 0, 32ull * n, 1);
                                const Bytes c = hh ? mark(hh, 0, (uint64_t)hl * n, 1) : Bytes();
                                want = meets(a, b) || meets(a, c) || meets(b, c) ? NOISE_ERROR_INVALID_PARAM : NOISE_ERROR_NONE;
                            }
                            const int got = hs_check_split(action, n, hl, ptr(k1), ptr(k2), ptr(hh));
                            ++g_checks;
                            if (got != want) {
                                char d[160];
                                snprintf(d, sizeof(d), "action=%#x n=%u hl=%u k1=%" PRIu64 " k2=%" PRIu64 " hh=%" PRIu64 ": got %#x want %#x",
                                         action, n, hl, k1, k2, hh, got, want);
                                fail("split check", d);
                            }
                        }
}

/* noise_aead_dev_handshake_new: the key each role must bring, the strides */
static void check_configs()
{
    struct Case { const char *name; int role; bool ls, le, rs, psk; uint64_t stride; int want; };
    const int I = NOISE_ROLE_INITIATOR, R = NOISE_ROLE_RESPONDER;
    const Case cases[] = {
        {"Noise_XX_25519_ChaChaPoly_SHA256", I, true, true, false, false, 32, 0},
        {"Noise_XX_25519_ChaChaPoly_SHA256", I, false, true, false, false, 32, NOISE_ERROR_LOCAL_KEY_REQUIRED},
        {"Noise_XX_25519_ChaChaPoly_SHA256", R, true, false, false, false, 32, NOISE_ERROR_LOCAL_KEY_REQUIRED},
        {"Noise_NN_25519_ChaChaPoly_SHA256", R, false, true, false, false, 0, 0},
        {"Noise_NN_25519_ChaChaPoly_SHA256", R, false, true, false, false, 31, NOISE_ERROR_INVALID_PARAM},
        {"Noise_NN_25519_ChaChaPoly_SHA256", R, false, true, false, false, 1, NOISE_ERROR_INVALID_PARAM},
        {"Noise_N_25519_AESGCM_BLAKE2b", R, true, false, false, false, 32, 0}, /* a one-way responder sends no e */
        {"Noise_N_25519_AESGCM_BLAKE2b", I, false, true, false, false, 32, NOISE_ERROR_REMOTE_KEY_REQUIRED},
        {"Noise_IK_25519_AESGCM_BLAKE2b", I, true, true, true, false, 40, 0},
        {"Noise_KK_25519_AESGCM_BLAKE2b", R, true, true, false, false, 32, NOISE_ERROR_REMOTE_KEY_REQUIRED},
        {"NoisePSK_NN_25519_AESGCM_BLAKE2b", I, false, true, false, false, 32, NOISE_ERROR_PSK_REQUIRED},
        {"NoisePSK_NN_25519_AESGCM_BLAKE2b", I, false, true, false, true, 32, 0},
        {"Noise_NN_25519_AESGCM_BLAKE2b", 0, false, true, false, false, 32, NOISE_ERROR_INVALID_PARAM},
        {"Noise_NN_448_AESGCM_BLAKE2b", I, false, true, false, false, 32, NOISE_ERROR_NOT_APPLICABLE},
        {"Noise_NN_25519_AESGCM", I, false, true, false, false, 32, NOISE_ERROR_UNKNOWN_NAME},
    };
    for (const Case &c : cases) {
        NoiseAeadHandshakeConfig cfg = {};
        cfg.protocol_name = c.name;
        cfg.role = c.role;
        cfg.n = 3;
        const uint8_t *key = (const uint8_t *)ptr(4096);
        if (c.ls) cfg.d_local_static_priv = key;
        if (c.le) cfg.d_local_ephemeral_priv = key;
        if (c.rs) cfg.d_remote_static_pub = key;
        if (c.psk) cfg.d_psk = key;
        cfg.local_static_stride = cfg.local_ephemeral_stride = cfg.remote_static_stride = cfg.psk_stride = c.stride;
        HsName name;
        ++g_checks;
        if (hs_check_config(&cfg, &name) != c.want) fail("config", c.name);
    }
    ++g_checks;
    HsName name;
    if (hs_check_config(nullptr, &name) != NOISE_ERROR_INVALID_PARAM) fail("config", "NULL");
}

int main()
{
    print_plans();
    answer_names();
    check_messages();
    check_splits();
    check_configs();
    printf("handshake_check: %ld plans %ld names %ld checks %ld failures\n", g_plans, g_names, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
