/*
 * handshake_plan.h — the host-only half of the batched Noise handshake
 * (include/noise_aead_hip.h section 8): the protocol-name parser, the token
 * table of the fifteen one-way and interactive patterns, the ordered steps and
 * the overhead of every message for (pattern, role, prefix, message index),
 * the argument checks of the entry points, and the length rule of one session
 * of a ragged call (hs_session_len, which the kernels run too), and the Noise
 * Pipes fallback (header section 15): XXfallback as a pattern of its own, its
 * name, who takes part (hs_fallback_takes, which the kernel runs too), the
 * merge rule and the argument checks of the two calls
 * (asan/handshake_fallback_check.cpp, tests/test_handshake_fallback_host.py),
 * and the sessions that change their object (header section 16): the rule of
 * one entry of a move (hs_move_rule, which the kernel runs too), the position
 * two objects must share and the argument checks of _new_like, _move and _drop
 * (asan/handshake_move_check.cpp, tests/test_handshake_move_host.py).
 *
 * No HIP header is included and no device pointer is dereferenced, so all of
 * it compiles with a host compiler alone and runs under ASan/UBSan
 * (asan/handshake_check.cpp, tests/test_handshake_host.py;
 * asan/handshake_ragged_check.cpp, tests/test_handshake_ragged_host.py) — in
 * the manner of dispatch.h.  handshake.hip turns the steps into launches.
 *
 * The table is the Noise specification's (section 7); the parser follows the
 * name grammar prefix_pattern_dh_cipher_hash.  The old-style "NoisePSK" prefix
 * is the one of noise-c v0.0.1: HKDF(ck, psk) after the prologue, and every
 * `e` token is also a MixKey of the ephemeral public key.
 */
#pragma once
#include "noise_aead_hip.h"

#include <stdint.h>
#include <string.h>

namespace na {

enum HsTok : uint8_t { HT_E, HT_S, HT_EE, HT_ES, HT_SE, HT_SS };

constexpr int HS_MAX_MSGS = 3, HS_MAX_TOKS = 5, HS_MAX_STEPS = HS_MAX_TOKS + 1;
constexpr uint32_t HS_DH_LEN = 32, HS_MAC_LEN = 16;

struct HsPattern {
    const char *name;
    bool pre_i_s, pre_r_s; /* the initiator's / responder's static key is a pre-message */
    uint8_t n_msgs;
    uint8_t n_toks[HS_MAX_MSGS];
    HsTok toks[HS_MAX_MSGS][HS_MAX_TOKS];
    bool pre_r_e; /* the responder's ephemeral key is a pre-message (HS_XXFALLBACK alone) */
};

/* initiator pre-message | responder pre-message | messages (-> <- -> ...) */
constexpr HsPattern HS_PATTERNS[] = {
    {"N", false, true, 1, {2}, {{HT_E, HT_ES}}},
    {"K", true, true, 1, {3}, {{HT_E, HT_ES, HT_SS}}},
    {"X", false, true, 1, {4}, {{HT_E, HT_ES, HT_S, HT_SS}}},
    {"NN", false, false, 2, {1, 2}, {{HT_E}, {HT_E, HT_EE}}},
    {"NK", false, true, 2, {2, 2}, {{HT_E, HT_ES}, {HT_E, HT_EE}}},
    {"NX", false, false, 2, {1, 4}, {{HT_E}, {HT_E, HT_EE, HT_S, HT_ES}}},
    {"XN", false, false, 3, {1, 2, 2}, {{HT_E}, {HT_E, HT_EE}, {HT_S, HT_SE}}},
    {"XK", false, true, 3, {2, 2, 2}, {{HT_E, HT_ES}, {HT_E, HT_EE}, {HT_S, HT_SE}}},
    {"XX", false, false, 3, {1, 4, 2}, {{HT_E}, {HT_E, HT_EE, HT_S, HT_ES}, {HT_S, HT_SE}}},
    {"KN", true, false, 2, {1, 3}, {{HT_E}, {HT_E, HT_EE, HT_SE}}},
    {"KK", true, true, 2, {3, 3}, {{HT_E, HT_ES, HT_SS}, {HT_E, HT_EE, HT_SE}}},
    {"KX", true, false, 2, {1, 5}, {{HT_E}, {HT_E, HT_EE, HT_SE, HT_S, HT_ES}}},
    {"IN", false, false, 2, {2, 3}, {{HT_E, HT_S}, {HT_E, HT_EE, HT_SE}}},
    {"IK", false, true, 2, {4, 3}, {{HT_E, HT_ES, HT_S, HT_SS}, {HT_E, HT_EE, HT_SE}}},
    {"IX", false, false, 2, {2, 5}, {{HT_E, HT_S}, {HT_E, HT_EE, HT_SE, HT_S, HT_ES}}},
};
constexpr int HS_N_PATTERNS = (int)(sizeof(HS_PATTERNS) / sizeof(HS_PATTERNS[0]));

/* XXfallback as the reference has it (patterns.c:444-471), the roles swapped
   against the handshake it follows: pre-message <- e, then -> e, ee, s, se and
   <- s, es.  Not a row of HS_PATTERNS: no name reaches it (hs_parse_name walks
   that table and refuses "XXfallback"); noise_aead_dev_handshake_fallback
   makes it of a running handshake (the end of this file). */
constexpr HsPattern HS_XXFALLBACK = {"XXfallback", false, false, 2, {4, 2}, {{HT_E, HT_EE, HT_S, HT_SE}, {HT_S, HT_ES}},
                                     true};

/* ------------------------------------------------------------ name parser */

struct HsName {
    int pattern; /* index into HS_PATTERNS */
    int cipher_id, hash_id;
    bool psk;
};

inline bool hs_field_is(const char *f, size_t n, const char *word) { return strlen(word) == n && !memcmp(f, word, n); }

inline int hs_find_pattern(const char *f, size_t n)
{
    for (int i = 0; i < HS_N_PATTERNS; ++i)
        if (hs_field_is(f, n, HS_PATTERNS[i].name)) return i;
    return -1;
}

/* a DH field this library knows of: 1 Curve25519, 2 one it does not compute
   (Curve448, NewHope), 0 no DH name */
inline int hs_dh_word(const char *f, size_t n)
{
    if (hs_field_is(f, n, "25519")) return 1;
    return hs_field_is(f, n, "448") || hs_field_is(f, n, "NewHope") ? 2 : 0;
}

/* prefix_pattern_dh_cipher_hash.  NOISE_ERROR_NONE and *out for the names in
   scope; NOISE_ERROR_NOT_APPLICABLE for a well-formed name that needs
   Curve448, NewHope, a hybrid ("hfs") pattern or XXfallback;
   NOISE_ERROR_UNKNOWN_NAME for everything else. */
inline int hs_parse_name(const char *name, HsName *out)
{
    if (!name || !out) return NOISE_ERROR_INVALID_PARAM;
    const char *f[5];
    size_t n[5];
    int nf = 0;
    const char *p = name;
    for (;;) {
        const char *u = strchr(p, '_');
        if (nf == 5) return NOISE_ERROR_UNKNOWN_NAME;
        f[nf] = p;
        n[nf] = u ? (size_t)(u - p) : strlen(p);
        ++nf;
        if (!u) break;
        p = u + 1;
    }
    if (nf != 5) return NOISE_ERROR_UNKNOWN_NAME;
    bool unsupported = false;
    HsName r = {};
    if (hs_field_is(f[0], n[0], "NoisePSK")) r.psk = true;
    else if (!hs_field_is(f[0], n[0], "Noise")) return NOISE_ERROR_UNKNOWN_NAME;
    /* pattern: one of the fifteen or XXfallback, then an optional hybrid
       modifier ("hfs" after a base pattern, "+hfs" after "fallback") */
    {
        size_t len = n[1];
        const bool hfs = len > 3 && !memcmp(f[1] + len - 3, "hfs", 3);
        if (hfs) len -= 3;
        bool fallback = false;
        if (hfs && len > 1 && f[1][len - 1] == '+') {
            --len;
            fallback = true; /* "+hfs" only follows another modifier */
        }
        if (hs_field_is(f[1], len, "XXfallback")) {
            unsupported = true;
        } else if (fallback) {
            return NOISE_ERROR_UNKNOWN_NAME;
        } else {
            r.pattern = hs_find_pattern(f[1], len);
            if (r.pattern < 0) return NOISE_ERROR_UNKNOWN_NAME;
            if (hfs) unsupported = true;
        }
    }
    /* dh: one name, or two joined by '+' (a hybrid's second exchange) */
    {
        const char *plus = (const char *)memchr(f[2], '+', n[2]);
        const size_t a = plus ? (size_t)(plus - f[2]) : n[2];
        const int w = hs_dh_word(f[2], a);
        if (!w) return NOISE_ERROR_UNKNOWN_NAME;
        if (w != 1) unsupported = true;
        if (plus) {
            if (!hs_dh_word(plus + 1, n[2] - a - 1)) return NOISE_ERROR_UNKNOWN_NAME;
            unsupported = true;
        }
    }
    if (hs_field_is(f[3], n[3], "ChaChaPoly")) r.cipher_id = NOISE_CIPHER_CHACHAPOLY;
    else if (hs_field_is(f[3], n[3], "AESGCM")) r.cipher_id = NOISE_CIPHER_AESGCM;
    else return NOISE_ERROR_UNKNOWN_NAME;
    if (hs_field_is(f[4], n[4], "BLAKE2s")) r.hash_id = NOISE_HASH_BLAKE2s;
    else if (hs_field_is(f[4], n[4], "BLAKE2b")) r.hash_id = NOISE_HASH_BLAKE2b;
    else if (hs_field_is(f[4], n[4], "SHA256")) r.hash_id = NOISE_HASH_SHA256;
    else if (hs_field_is(f[4], n[4], "SHA512")) r.hash_id = NOISE_HASH_SHA512;
    else return NOISE_ERROR_UNKNOWN_NAME;
    if (unsupported) return NOISE_ERROR_NOT_APPLICABLE;
    *out = r;
    return NOISE_ERROR_NONE;
}

/* ------------------------------------------------------------------ steps */

enum HsStepKind : uint8_t {
    HS_STEP_E,       /* the ephemeral public key, in the clear; mix_key under NoisePSK */
    HS_STEP_S,       /* the static public key through encrypt/decrypt_and_hash */
    HS_STEP_DH,      /* a ladder launch and MixKey of its output */
    HS_STEP_PAYLOAD, /* the payload through encrypt/decrypt_and_hash */
};

struct HsStep {
    HsStepKind kind;
    HsTok tok;                /* E, S, DH */
    bool keyed;               /* S, PAYLOAD: a key is set, so AEAD and 16 more bytes */
    bool mix_key;             /* E: NoisePSK */
    bool priv_static;         /* DH: the local static key (else the local ephemeral) */
    bool pub_static;          /* DH: the remote static key (else the remote ephemeral) */
};

struct HsMessage {
    int n_steps;
    HsStep steps[HS_MAX_STEPS];
    uint32_t overhead; /* bytes the message adds to its payload */
    bool keyed_after;
    int next_action;   /* of the role the plan was made for */
};

inline bool hs_is_initiator(int role) { return role == NOISE_ROLE_INITIATOR; }

/* whether a key is set when message `index` starts: a DH token, or an `e`
   under NoisePSK, of an earlier message set it (the PSK start-up step itself
   sets none); a pre-message `e` under NoisePSK set it before message 0
   (handshakestate.c:854-857, :870-873) */
inline bool hs_keyed_before(const HsPattern &p, bool psk, int index)
{
    if (psk && p.pre_r_e) return true;
    for (int m = 0; m < index && m < p.n_msgs; ++m)
        for (int t = 0; t < p.n_toks[m]; ++t)
            if (p.toks[m][t] >= HT_EE || (psk && p.toks[m][t] == HT_E)) return true;
    return false;
}

/* Message `index` (0: the initiator's first) as `role` sees it, whether it
   writes or reads it; keyed: hs_keyed_before. */
inline HsMessage hs_message(const HsPattern &p, int role, bool psk, int index, bool keyed)
{
    HsMessage m = {};
    const bool init = hs_is_initiator(role);
    for (int t = 0; t < p.n_toks[index]; ++t) {
        HsStep s = {};
        s.tok = p.toks[index][t];
        switch (s.tok) {
        case HT_E:
            s.kind = HS_STEP_E;
            s.mix_key = psk;
            m.overhead += HS_DH_LEN;
            if (psk) keyed = true;
            break;
        case HT_S:
            s.kind = HS_STEP_S;
            s.keyed = keyed;
            m.overhead += HS_DH_LEN + (keyed ? HS_MAC_LEN : 0);
            break;
        default:
            s.kind = HS_STEP_DH;
            s.priv_static = s.tok == HT_SS || s.tok == (init ? HT_SE : HT_ES);
            s.pub_static = s.tok == HT_SS || s.tok == (init ? HT_ES : HT_SE);
            keyed = true;
            break;
        }
        m.steps[m.n_steps++] = s;
    }
    HsStep pl = {};
    pl.kind = HS_STEP_PAYLOAD;
    pl.keyed = keyed;
    m.overhead += keyed ? HS_MAC_LEN : 0;
    m.steps[m.n_steps++] = pl;
    m.keyed_after = keyed;
    if (index + 1 == p.n_msgs) m.next_action = NOISE_ACTION_SPLIT;
    else m.next_action = ((index + 1) % 2 == 0) == init ? NOISE_ACTION_WRITE_MESSAGE : NOISE_ACTION_READ_MESSAGE;
    return m;
}

/* the first action of a role */
inline int hs_first_action(int role)
{
    return hs_is_initiator(role) ? NOISE_ACTION_WRITE_MESSAGE : NOISE_ACTION_READ_MESSAGE;
}

/* What a role must bring: its static key pair when it has a pre-message `s`
   or sends an `s` token, its ephemeral private key when it sends an `e`, the
   remote static public key when the other side's `s` is a pre-message.  A
   pre-message `e` of the responder is an ephemeral key pair the responder
   brings and a remote ephemeral public key the initiator brings. */
struct HsNeeds {
    bool local_static, local_ephemeral, remote_static, remote_ephemeral;
};

inline HsNeeds hs_needs(const HsPattern &p, int role)
{
    const bool init = hs_is_initiator(role);
    HsNeeds r = {init ? p.pre_i_s : p.pre_r_s, p.pre_r_e && !init, init ? p.pre_r_s : p.pre_i_s, p.pre_r_e && init};
    for (int m = init ? 0 : 1; m < p.n_msgs; m += 2)
        for (int t = 0; t < p.n_toks[m]; ++t) {
            if (p.toks[m][t] == HT_S) r.local_static = true;
            if (p.toks[m][t] == HT_E) r.local_ephemeral = true;
        }
    return r;
}

/* --------------------------------------------------------- argument checks
   Pointers are compared as numbers and never dereferenced. */

typedef unsigned __int128 hs_u128;

inline bool hs_key_stride_ok(uint64_t stride) { return stride == 0 || stride >= HS_DH_LEN; }

/* [p, p + (n - 1) * stride + len) of an input (stride 0: one value) meets
   the same of an output */
inline bool hs_spans_meet(const void *in, uint64_t in_stride, uint64_t in_len, const void *out, uint64_t out_stride,
                          uint64_t out_len, uint32_t n)
{
    if (!n || !in_len || !out_len) return false;
    const hs_u128 a = (uintptr_t)in, b = (uintptr_t)out;
    const hs_u128 a_hi = a + (hs_u128)(n - 1) * in_stride + in_len, b_hi = b + (hs_u128)(n - 1) * out_stride + out_len;
    return a < b_hi && b < a_hi;
}

/* noise_aead_dev_handshake_new: the configuration against the parsed name */
inline int hs_check_config(const NoiseAeadHandshakeConfig *cfg, HsName *name)
{
    if (!cfg || !name || !cfg->protocol_name) return NOISE_ERROR_INVALID_PARAM;
    const int rc = hs_parse_name(cfg->protocol_name, name);
    if (rc) return rc;
    if (cfg->role != NOISE_ROLE_INITIATOR && cfg->role != NOISE_ROLE_RESPONDER) return NOISE_ERROR_INVALID_PARAM;
    const HsNeeds need = hs_needs(HS_PATTERNS[name->pattern], cfg->role);
    if ((need.local_static && !cfg->d_local_static_priv) || (need.local_ephemeral && !cfg->d_local_ephemeral_priv))
        return NOISE_ERROR_LOCAL_KEY_REQUIRED;
    if (need.remote_static && !cfg->d_remote_static_pub) return NOISE_ERROR_REMOTE_KEY_REQUIRED;
    if (name->psk && !cfg->d_psk) return NOISE_ERROR_PSK_REQUIRED;
    if (cfg->prologue_len && !cfg->d_prologue) return NOISE_ERROR_INVALID_PARAM;
    if (cfg->prologue_len && cfg->prologue_stride && cfg->prologue_stride < cfg->prologue_len)
        return NOISE_ERROR_INVALID_PARAM;
    if ((name->psk && !hs_key_stride_ok(cfg->psk_stride)) ||
        (need.local_static && !hs_key_stride_ok(cfg->local_static_stride)) ||
        (need.local_ephemeral && !hs_key_stride_ok(cfg->local_ephemeral_stride)) ||
        (need.remote_static && !hs_key_stride_ok(cfg->remote_static_stride)))
        return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* noise_aead_dev_handshake_write_message; NOISE_ERROR_NONE with n == 0 once
   the state and the lengths are right */
inline int hs_check_write(int action, uint32_t n, uint32_t overhead, const void *d_payload, uint64_t payload_stride,
                          uint32_t payload_len, const void *d_msg, uint64_t msg_stride)
{
    if (action != NOISE_ACTION_WRITE_MESSAGE) return NOISE_ERROR_INVALID_STATE;
    if ((uint64_t)payload_len + overhead > NOISE_MAX_PAYLOAD_LEN) return NOISE_ERROR_INVALID_LENGTH;
    if (!n) return NOISE_ERROR_NONE;
    const uint32_t msg_len = payload_len + overhead;
    if (!d_msg || (payload_len && !d_payload)) return NOISE_ERROR_INVALID_PARAM;
    if (msg_stride < msg_len) return NOISE_ERROR_INVALID_PARAM;
    if (payload_len && payload_stride && payload_stride < payload_len) return NOISE_ERROR_INVALID_PARAM;
    if (hs_spans_meet(d_payload, payload_stride, payload_len, d_msg, msg_stride, msg_len, n)) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* noise_aead_dev_handshake_read_message */
inline int hs_check_read(int action, uint32_t n, uint32_t overhead, const void *d_msg, uint64_t msg_stride,
                         uint32_t msg_len, const void *d_payload, uint64_t payload_stride)
{
    if (action != NOISE_ACTION_READ_MESSAGE) return NOISE_ERROR_INVALID_STATE;
    if (msg_len > NOISE_MAX_PAYLOAD_LEN || msg_len < overhead) return NOISE_ERROR_INVALID_LENGTH;
    if (!n) return NOISE_ERROR_NONE;
    const uint32_t payload_len = msg_len - overhead;
    if (!d_msg || (payload_len && !d_payload)) return NOISE_ERROR_INVALID_PARAM;
    if (msg_stride && msg_stride < msg_len) return NOISE_ERROR_INVALID_PARAM;
    if (payload_len && payload_stride < payload_len) return NOISE_ERROR_INVALID_PARAM;
    if (hs_spans_meet(d_msg, msg_stride, msg_len, d_payload, payload_stride, payload_len, n)) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* ------------------------------------------------- per-session lengths
   The ragged calls (_write_message_ragged, _read_message_ragged) give every
   session its own length.  One source for both compilers, as tr_walk is
   (transport_plan.h): hipcc's device pass builds the kernels of handshake.hip
   from hs_session_len, plain g++ builds asan/handshake_ragged_check.cpp from
   it. */

#if defined(__HIPCC__)
#define HS_FN __host__ __device__ __forceinline__
#else
#define HS_FN static inline __attribute__((always_inline))
#endif

constexpr uint8_t HS_STATUS_LENGTH = 4; /* NOISE_ERROR_INVALID_LENGTH of one session */

struct HsLen {
    bool refused;   /* the session takes status 4 and nothing of it is read or written */
    uint32_t other; /* write: the message length; read: the payload length; 0 when refused */
};

/* What hs_check_write / hs_check_read refuse for a whole batch, for one
   session: write takes the payload length and refuses a message over 65535
   bytes; read takes the message length and refuses one over 65535 bytes or
   below the overhead (handshakestate.c:1320-1324, :1454, :1489;
   symmetricstate.c:419-422). */
HS_FN HsLen hs_session_len(uint32_t overhead, uint32_t len, bool write)
{
    HsLen r = {true, 0};
    if (write) {
        if ((uint64_t)len + overhead > NOISE_MAX_PAYLOAD_LEN) return r;
        r.other = len + overhead;
    } else {
        if (len > NOISE_MAX_PAYLOAD_LEN || len < overhead) return r;
        r.other = len - overhead;
    }
    r.refused = false;
    return r;
}

/* [a, a + a_bytes) meets [b, b + b_bytes) */
inline bool hs_ranges_meet(const void *a, hs_u128 a_bytes, const void *b, hs_u128 b_bytes)
{
    if (!a_bytes || !b_bytes) return false;
    const hs_u128 x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

/* the output length array of a ragged call against the arrays the call reads */
inline bool hs_out_len_meets(const void *d_out_len, const void *d_off_a, const void *d_off_b, const void *d_in_len,
                             uint32_t n)
{
    const hs_u128 lb = (hs_u128)4 * n, ob = (hs_u128)8 * n;
    return hs_ranges_meet(d_out_len, lb, d_off_a, d_off_a ? ob : 0) ||
           hs_ranges_meet(d_out_len, lb, d_off_b, d_off_b ? ob : 0) ||
           hs_ranges_meet(d_out_len, lb, d_in_len, d_in_len ? lb : 0);
}

/* noise_aead_dev_handshake_write_message_ragged, in the order of the header;
   the payload triple may be NULL all three together (every payload empty) */
inline int hs_check_write_ragged(const void *hs, int action, uint32_t n, const void *d_payload,
                                 const void *d_payload_off, const void *d_payload_len, const void *d_msg,
                                 const void *d_msg_off, const void *d_msg_len)
{
    if (!hs) return NOISE_ERROR_INVALID_PARAM;
    if (action != NOISE_ACTION_WRITE_MESSAGE) return NOISE_ERROR_INVALID_STATE;
    if (!n) return NOISE_ERROR_NONE;
    if (!d_msg || !d_msg_off || !d_msg_len) return NOISE_ERROR_INVALID_PARAM;
    const int given = (d_payload != nullptr) + (d_payload_off != nullptr) + (d_payload_len != nullptr);
    if (given != 0 && given != 3) return NOISE_ERROR_INVALID_PARAM;
    if (hs_out_len_meets(d_msg_len, d_payload_off, d_msg_off, d_payload_len, n)) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* noise_aead_dev_handshake_read_message_ragged */
inline int hs_check_read_ragged(const void *hs, int action, uint32_t n, const void *d_msg, const void *d_msg_off,
                                const void *d_msg_len, const void *d_payload, const void *d_payload_off,
                                const void *d_payload_len)
{
    if (!hs) return NOISE_ERROR_INVALID_PARAM;
    if (action != NOISE_ACTION_READ_MESSAGE) return NOISE_ERROR_INVALID_STATE;
    if (!n) return NOISE_ERROR_NONE;
    if (!d_msg || !d_msg_off || !d_msg_len || !d_payload || !d_payload_off || !d_payload_len)
        return NOISE_ERROR_INVALID_PARAM;
    if (hs_out_len_meets(d_payload_len, d_msg_off, d_payload_off, d_msg_len, n)) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* noise_aead_dev_handshake_split: the three packed outputs must be disjoint */
inline int hs_check_split(int action, uint32_t n, uint32_t hash_len, const void *d_k1, const void *d_k2,
                          const void *d_hh)
{
    if (action != NOISE_ACTION_SPLIT) return NOISE_ERROR_INVALID_STATE;
    if (!n) return NOISE_ERROR_NONE;
    if (!d_k1 || !d_k2) return NOISE_ERROR_INVALID_PARAM;
    const uint64_t kb = 32ull * n, hb = (uint64_t)hash_len * n;
    if (hs_spans_meet(d_k1, 0, kb, d_k2, 0, kb, 1)) return NOISE_ERROR_INVALID_PARAM;
    if (d_hh && (hs_spans_meet(d_k1, 0, kb, d_hh, 0, hb, 1) || hs_spans_meet(d_k2, 0, kb, d_hh, 0, hb, 1)))
        return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* ------------------------------------------------- the Noise Pipes fallback
   noise_aead_dev_handshake_fallback / _fallback_merge (header section 15):
   the new name, the patterns it may follow, which sessions take part — one
   statement for both compilers, run by the hs_fallback_take kernel of
   handshake.hip and by asan/handshake_fallback_check.cpp — and the argument
   checks of the two calls. */

constexpr uint8_t HS_STATUS_ABSENT = 5; /* "not in this object" */
constexpr size_t HS_NAME_MAX = 64;      /* the longest name, a NoisePSK XXfallback one, has 44 characters */

/* the name of `name`'s handshake with the pattern field replaced by
   XXfallback; the length, 0 when it does not fit in cap bytes with its NUL */
inline size_t hs_fallback_name(const HsName &name, char *out, size_t cap)
{
    const char *hash = name.hash_id == NOISE_HASH_BLAKE2s   ? "BLAKE2s"
                       : name.hash_id == NOISE_HASH_BLAKE2b ? "BLAKE2b"
                       : name.hash_id == NOISE_HASH_SHA256  ? "SHA256"
                                                            : "SHA512";
    const char *parts[] = {name.psk ? "NoisePSK" : "Noise", "_", HS_XXFALLBACK.name, "_25519_",
                           name.cipher_id == NOISE_CIPHER_AESGCM ? "AESGCM" : "ChaChaPoly", "_", hash};
    size_t len = 0;
    for (const char *p : parts) {
        const size_t n = strlen(p);
        if (len + n >= cap) return 0;
        memcpy(out + len, p, n);
        len += n;
    }
    out[len] = 0;
    return len;
}

/* NOISE_REQ_FALLBACK_POSSIBLE: interactive, the responder's static key known
   beforehand */
inline bool hs_fallback_possible(const HsPattern &p) { return p.n_msgs >= 2 && p.pre_r_s; }

/* A former responder falls back after a first message that failed (1) or that
   verified (0: "it decides to always fall back anyway",
   handshakestate.c:1001-1005), a former initiator after writing it (0).  A
   session of status 3 or 4 never received or kept a usable e. */
HS_FN bool hs_fallback_eligible(uint8_t status, bool was_initiator)
{
    return status == 0 || (status == 1 && !was_initiator);
}

/* whether a session of that status in the original handshake takes part in
   the fallback; selected: d_select is NULL or the session's byte is not 0 */
HS_FN bool hs_fallback_takes(uint8_t status, bool selected, uint32_t flags, bool was_initiator)
{
    if (!hs_fallback_eligible(status, was_initiator) || !selected) return false;
    return (flags & NOISE_AEAD_FALLBACK_ONLY_FAILED) ? status == 1 : true;
}

/* what _fallback_merge does with a session by its status in the fallback */
enum HsMerge : uint8_t { HS_MERGE_TAKE, HS_MERGE_KEEP, HS_MERGE_ZERO };

HS_FN HsMerge hs_fallback_merge_rule(uint8_t fb_status)
{
    return fb_status == 0 ? HS_MERGE_TAKE : (fb_status == HS_STATUS_ABSENT ? HS_MERGE_KEEP : HS_MERGE_ZERO);
}

/* the handshake a fallback is asked of, as the host object knows it */
struct HsFallbackFrom {
    const HsPattern *pattern; /* NULL: no object */
    bool psk;
    int role, action, index;  /* index: messages done */
    bool has_static;          /* a static private key was given to _new */
    bool made_like = false;   /* the object came from _new_like (section 16): it owns its private-key rows */
};

/* noise_aead_dev_handshake_fallback, in the order of the header */
inline int hs_check_fallback(const HsFallbackFrom &from, const NoiseAeadHandshakeFallbackConfig *cfg, const void *fb)
{
    if (!from.pattern || !cfg || !fb) return NOISE_ERROR_INVALID_PARAM;
    if (from.pattern->pre_r_e || !hs_fallback_possible(*from.pattern) || from.made_like) return NOISE_ERROR_NOT_APPLICABLE;
    const bool init = hs_is_initiator(from.role);
    if (from.index != 1 || from.action != (init ? NOISE_ACTION_READ_MESSAGE : NOISE_ACTION_WRITE_MESSAGE))
        return NOISE_ERROR_INVALID_STATE;
    if (!from.has_static || (!init && !cfg->d_local_ephemeral_priv)) return NOISE_ERROR_LOCAL_KEY_REQUIRED;
    if (from.psk && !cfg->d_psk) return NOISE_ERROR_PSK_REQUIRED;
    if (cfg->prologue_len && !cfg->d_prologue) return NOISE_ERROR_INVALID_PARAM;
    if (cfg->prologue_len && cfg->prologue_stride && cfg->prologue_stride < cfg->prologue_len)
        return NOISE_ERROR_INVALID_PARAM;
    if ((from.psk && !hs_key_stride_ok(cfg->psk_stride)) || (!init && !hs_key_stride_ok(cfg->local_ephemeral_stride)))
        return NOISE_ERROR_INVALID_PARAM;
    if (cfg->flags & ~NOISE_AEAD_FALLBACK_ONLY_FAILED) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* noise_aead_dev_handshake_fallback_merge: the outputs (32n, 32n, hash_len * n
   and n bytes) against every array the call reads (d_fb_status: the
   fallback's own statuses) */
inline int hs_check_fallback_merge(const void *fb, int action, uint32_t n, uint32_t hash_len, const void *d_fb_status,
                                   const void *d_hs_status, const void *d_k1, const void *d_k2, const void *d_fb_k1,
                                   const void *d_fb_k2, const void *d_h, const void *d_fb_h, const void *d_status)
{
    if (!fb || !d_hs_status || !d_k1 || !d_k2 || !d_fb_k1 || !d_fb_k2 || !d_status || (!d_h != !d_fb_h))
        return NOISE_ERROR_INVALID_PARAM;
    if (action != NOISE_ACTION_COMPLETE) return NOISE_ERROR_INVALID_STATE;
    if (!n) return NOISE_ERROR_NONE;
    const hs_u128 kb = (hs_u128)32 * n, hb = (hs_u128)hash_len * n;
    const void *outs[] = {d_k1, d_k2, d_h, d_status}, *ins[] = {d_fb_k1, d_fb_k2, d_fb_h, d_hs_status, d_fb_status};
    const hs_u128 out_bytes[] = {kb, kb, d_h ? hb : 0, n}, in_bytes[] = {kb, kb, d_fb_h ? hb : 0, n, d_fb_status ? n : 0};
    for (int o = 0; o < 4; ++o)
        for (int i = 0; i < 5; ++i)
            if (hs_ranges_meet(outs[o], out_bytes[o], ins[i], in_bytes[i])) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* ------------------------------------------ sessions that change their object
   noise_aead_dev_handshake_new_like / _move / _drop (header section 16): the
   rule of one entry of a move — one statement for both compilers, run by the
   hs_move kernel of handshake.hip and by asan/handshake_move_check.cpp — what
   "the same position" means, and the argument checks of the three calls. */

/* The outcome of entry j, the byte _move writes to d_result[j].  The causes
   are tested in this order; the statuses are not looked at (and the kernel
   reads none) unless both lane numbers are in range. */
HS_FN uint8_t hs_move_rule(bool src_in_range, bool dst_in_range, uint8_t src_status, uint8_t dst_status)
{
    if (!src_in_range || !dst_in_range) return NOISE_AEAD_MOVE_RANGE;
    if (src_status == HS_STATUS_ABSENT) return NOISE_AEAD_MOVE_EMPTY;
    if (dst_status != HS_STATUS_ABSENT) return NOISE_AEAD_MOVE_TAKEN;
    return NOISE_AEAD_MOVED;
}

/* everything of an object that is the same for all its sessions and lives on
   the host: where it stands in which handshake */
struct HsPosition {
    HsName name;
    bool fallback;
    int role, action, index;
    bool keyed;
    uint64_t nonce;
};

inline bool hs_same_position(const HsPosition &a, const HsPosition &b)
{
    return a.name.pattern == b.name.pattern && a.name.cipher_id == b.name.cipher_id && a.name.hash_id == b.name.hash_id &&
           a.name.psk == b.name.psk && a.fallback == b.fallback && a.role == b.role && a.action == b.action &&
           a.index == b.index && a.keyed == b.keyed && a.nonce == b.nonce;
}

/* how an object holds one of its two private keys */
enum HsHold : uint8_t {
    HS_HOLD_NONE,   /* it never had it */
    HS_HOLD_SHARED, /* once for all: stride 0, the caller's memory */
    HS_HOLD_EACH,   /* per session: the caller's rows, or rows the object owns (_new_like) */
};

struct HsKey {
    HsHold hold;
    const void *ptr; /* compared for HS_HOLD_SHARED alone */
    bool owned;      /* HS_HOLD_EACH: the rows are the object's own */
};

inline HsHold hs_hold_of(const void *priv, uint64_t stride) { return !priv ? HS_HOLD_NONE : (stride ? HS_HOLD_EACH : HS_HOLD_SHARED); }

/* noise_aead_dev_handshake_new_like */
inline int hs_check_new_like(const void *out, const void *like, int action)
{
    if (!out || !like) return NOISE_ERROR_INVALID_PARAM;
    if (action != NOISE_ACTION_WRITE_MESSAGE && action != NOISE_ACTION_READ_MESSAGE && action != NOISE_ACTION_SPLIT)
        return NOISE_ERROR_INVALID_STATE;
    return NOISE_ERROR_NONE;
}

/* one object of a move, as the host knows it; pos and keys are not looked at when obj is NULL */
struct HsMoveSide {
    const void *obj;
    HsPosition pos;
    HsKey keys[2]; /* static, ephemeral */
    uint32_t n;
    const void *d_lanes;
};

/* noise_aead_dev_handshake_move, in the order of the header */
inline int hs_check_move(const HsMoveSide &dst, const HsMoveSide &src, uint32_t m, const void *d_result)
{
    if (!dst.obj || !src.obj) return NOISE_ERROR_INVALID_PARAM;
    if (dst.obj == src.obj) return NOISE_ERROR_INVALID_PARAM;
    const int action = src.pos.action;
    if (!hs_same_position(dst.pos, src.pos) ||
        (action != NOISE_ACTION_WRITE_MESSAGE && action != NOISE_ACTION_READ_MESSAGE && action != NOISE_ACTION_SPLIT))
        return NOISE_ERROR_INVALID_STATE;
    for (int k = 0; k < 2; ++k) {
        const HsKey &d = dst.keys[k], &s = src.keys[k];
        if (d.hold != s.hold) return NOISE_ERROR_INVALID_PARAM;
        if (d.hold == HS_HOLD_SHARED && d.ptr != s.ptr) return NOISE_ERROR_INVALID_PARAM;
        if (d.hold == HS_HOLD_EACH && !d.owned) return NOISE_ERROR_INVALID_PARAM; /* the caller's memory is never written */
    }
    if (!m) return NOISE_ERROR_NONE;
    if ((!dst.d_lanes && m > dst.n) || (!src.d_lanes && m > src.n)) return NOISE_ERROR_INVALID_PARAM;
    if (hs_ranges_meet(d_result, d_result ? m : 0, dst.d_lanes, dst.d_lanes ? (hs_u128)4 * m : 0) ||
        hs_ranges_meet(d_result, d_result ? m : 0, src.d_lanes, src.d_lanes ? (hs_u128)4 * m : 0))
        return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* noise_aead_dev_handshake_drop: as noise_aead_dev_transport_clear_keys (section 10) */
inline int hs_check_drop(const void *hs, uint32_t n, const void *d_lanes, uint32_t m)
{
    if (!hs) return NOISE_ERROR_INVALID_PARAM;
    if (!m) return NOISE_ERROR_NONE;
    if (m > n || !d_lanes) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

} // namespace na
