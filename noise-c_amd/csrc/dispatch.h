/*
 * dispatch.h — which kernel a job runs, and whether the job may run at all.
 * Host-only plain C++17 (no HIP include; g++ alone compiles it, as
 * worker_proto.h): the A/B switches, the job checks, the facts of a job and
 * one plan function per entry point, each rule written once.  aead_api.hip
 * checks, plans and hands the Plan to the launchers (launch_chacha.hip,
 * launch_aes.hip), which turn its kernel value into a function pointer.
 * asan/dispatch_check.cpp runs all of it on the CPU under ASan/UBSan and
 * compares the plans with tests/golden/dispatch_plans.txt.gz.
 */
#pragma once
#include "noise_aead_hip.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

namespace na {

/* Launch geometry the plans count with; the launchers static_assert these
   against the kernels' own constants. */
constexpr uint32_t PLAN_BLOCK = 256;      /* threads of every workgroup but the staged AES-GCM ones */
constexpr uint32_t PLAN_GCM_LANES = 4;    /* GCM_LANES */
constexpr uint32_t PLAN_GCM_WG = 1024;    /* GCM_WG */
constexpr uint32_t PLAN_GCM_WG_RECS = 256; /* GCM_WG_RECS */
constexpr uint32_t PLAN_SEG_KMAX = 16;    /* SEG_KMAX */

/* The length of a Noise hash (constants.h:43-46); 0 for an id that is none.
   The one place the host knows it: the entry points turn 0 into their answer
   for an unknown id and hand the kernels the length. */
inline uint32_t hash_len(int hash_id)
{
    switch (hash_id) {
    case NOISE_HASH_BLAKE2s: case NOISE_HASH_SHA256: return 32;
    case NOISE_HASH_BLAKE2b: case NOISE_HASH_SHA512: return 64;
    }
    return 0;
}

/* ------------------------------------------------------------ the switches
   env_flag: a switch that is on by default goes off with "0", one that is
   off goes on with "1"; env_int: a positive number, else dflt; env_choice:
   the 1-based place of the variable's value among `values`, else 0. */
inline bool env_flag(const char *name, bool on)
{
    const char *e = getenv(name);
    return e ? (on ? e[0] != '0' : e[0] == '1') : on;
}

inline int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e && atoi(e) > 0 ? atoi(e) : dflt;
}

inline int env_choice(const char *name, std::initializer_list<const char *> values)
{
    const char *e = getenv(name);
    int i = 0;
    for (const char *v : values) {
        ++i;
        if (e && !strcmp(e, v)) return i;
    }
    return 0;
}

/* The A/B switches of kernel choice (measurement runs; the defaults ship). */
struct Switches {
    /* NOISE_AEAD_SOLO=0 keeps the 4-lane kernels everywhere (no one lane per
       record from SOLO_MIN_RECORDS) */
    bool solo = true;
    /* NOISE_AEAD_SEG: the segmented kernels (chachapoly_seg.hip).  0 turns
       them off (the ragged path then keeps the windowed 8-lane kernels); 2
       also makes a standalone job of SOLO_MIN_RECORDS <= n <
       SOLO_MIN_STANDALONE FAST records take two segments per record (2048
       waves at 64 Ki records, two per SIMD).  Round 5 measured that shape
       slower than the four-lane staged kernel it would replace — C2
       standalone seal 73 vs 63 us (profiles/r05/seg2_standalone_ab.jsonl): 7 %
       fewer VALU instructions than four lanes but 16 % more than one lane
       per record (the split's second chain, r^e, the 24th block slot), and
       two waves of six steps per SIMD issue 11 % slower than the duplex
       launch's seal + open pair — so the default keeps four lanes there. */
    int seg = 1;
    /* NOISE_AEAD_CT_GHASH=1: NOISE_AEAD_FLAG_CT_GHASH for every job */
    bool ct_ghash = false;
    /* NOISE_AEAD_LANES=narrow: the host paths keep K <= 8 and the 4-lane AES
       kernels */
    bool lanes_narrow = false;
    /* NOISE_AEAD_DUPLEX_RUNS=0: chachapoly_duplex_solo alternates seal and
       open blocks one by one instead of in runs of the CU count */
    bool duplex_runs = true;
    /* NOISE_AEAD_GCM_SHAPE=w1024r1 | w1024r2 | w1024r2k8 (1, 2, 3) forces a
       ragged AES-GCM launch shape */
    int gcm_shape = 0;
    /* NOISE_AEAD_GCM_DUPLEX=staged selects gcm_duplex_staged over the fused
       duplex kernel (one LDS fill, seal then open per workgroup: C3
       +0.7-0.9 % in three interleaved rounds, profiles/r03/gcm_fused_ab.jsonl) */
    bool gcm_duplex_fused = true;
    /* NOISE_AEAD_RAGGED_DUPLEX: noise_aead_dev_duplex_ragged's shared
       launches.  0: every ragged duplex is two launches (seal, then open);
       1: every family that can share a launch does; unset (-1): each family's
       measured default (ragged_duplex_default) */
    int ragged_duplex = -1;
};

inline Switches switches_from_env()
{
    Switches s;
    s.solo = env_flag("NOISE_AEAD_SOLO", true);
    const char *seg = getenv("NOISE_AEAD_SEG");
    s.seg = seg ? (seg[0] == '0' ? 0 : (seg[0] == '2' ? 2 : 1)) : 1;
    s.ct_ghash = env_flag("NOISE_AEAD_CT_GHASH", false);
    s.lanes_narrow = env_choice("NOISE_AEAD_LANES", {"narrow"}) == 1;
    s.duplex_runs = env_flag("NOISE_AEAD_DUPLEX_RUNS", true);
    s.gcm_shape = env_choice("NOISE_AEAD_GCM_SHAPE", {"w1024r1", "w1024r2", "w1024r2k8"});
    s.gcm_duplex_fused = env_choice("NOISE_AEAD_GCM_DUPLEX", {"staged"}) != 1;
    const char *rd = getenv("NOISE_AEAD_RAGGED_DUPLEX");
    s.ragged_duplex = rd ? (rd[0] == '0' ? 0 : (rd[0] == '1' ? 1 : -1)) : -1;
    return s;
}

/* the process's switches, read from the environment once */
inline const Switches &switches()
{
    static const Switches s = switches_from_env();
    return s;
}

/* ------------------------------------------------------------ job checks
   Byte span [lo, hi) a uniform job's input (or output) records occupy.
   open = the job is an open (its input holds CT || tag).  All span
   arithmetic is 128-bit: no pointer, stride or record count overflows it. */
typedef unsigned __int128 u128;
typedef __int128 i128;

struct Span { u128 lo, hi; };

inline bool meet(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }

inline Span job_span(const NoiseAeadUniform *j, bool out, bool open)
{
    const u128 base = (uintptr_t)(out ? (const void *)j->out : (const void *)j->in);
    const u128 stride = out ? j->out_stride : j->in_stride;
    const u128 rec = (u128)j->len + ((out != open) ? 16u : 0u); /* CT || tag side */
    return {base, j->n_records ? base + (u128)(j->n_records - 1) * stride + rec : base};
}

/* [lo, hi) of a job's AD (lo == hi: none) and of its status array */
inline Span ad_span(const NoiseAeadUniform *j)
{
    const u128 lo = (uintptr_t)j->ad;
    return {lo, j->ad_len && j->n_records ? lo + (u128)(j->n_records - 1) * j->ad_stride + j->ad_len : lo};
}

inline Span status_span(const NoiseAeadUniform *j)
{
    const u128 lo = (uintptr_t)j->status;
    return {lo, j->status ? lo + j->n_records : lo};
}

inline i128 floor_div(i128 a, i128 b) { return a >= 0 ? a / b : -((-a + b - 1) / b); } /* b > 0 */

/* Does any input record [in + i s, in + i s + rin) meet any output record
   [out + k s, out + k s + rout), i, k < n, one stride s > 0 for both?  With
   d = out - in they meet iff some m = i - k, |m| < n, has
   d - rin < m s < d + rout. */
inline bool strided_records_meet(uint64_t in, uint64_t out, uint64_t s, uint64_t rin, uint64_t rout, uint32_t n)
{
    if (!rin || !rout || !n || !s) return false;
    const i128 d = (i128)out - (i128)in, st = (i128)s;
    const i128 m_lo = floor_div(d - (i128)rin, st) + 1;      /* smallest m with m s > d - rin */
    const i128 m_hi = -floor_div(-(d + (i128)rout), st) - 1; /* largest m with m s < d + rout */
    const i128 lim = (i128)n - 1;
    return (m_lo > -lim ? m_lo : -lim) <= (m_hi < lim ? m_hi : lim);
}

/* In-place jobs must be exactly in place (in == out, one stride): records
   whose input and output spans overlap any other way would race with their
   neighbours' reads (and a rejected record's scrub would wipe input other
   records still need). */
inline int check_uniform(const NoiseAeadUniform *j, bool open)
{
    if (!j || !j->ctx || !j->nonce_base || !j->in || !j->out || !j->recs_per_state)
        return NOISE_ERROR_INVALID_PARAM;
    if (j->ad_len && !j->ad) return NOISE_ERROR_INVALID_PARAM;
    if (j->len > NOISE_MAX_PAYLOAD_LEN - 16) return NOISE_ERROR_INVALID_LENGTH;
    if ((uintptr_t)j->ctx & 15) return NOISE_ERROR_INVALID_PARAM;
    if (j->n_records && !(j->in == j->out && j->in_stride == j->out_stride)) {
        /* records of one stride may interleave (input and output slots
           alternating in one buffer) as long as no two of them meet; other
           layouts need disjoint spans */
        const uint64_t rin = (uint64_t)j->len + (open ? 16u : 0u), rout = (uint64_t)j->len + (open ? 0u : 16u);
        if (j->in_stride == j->out_stride && j->in_stride >= rin && j->in_stride >= rout) {
            if (strided_records_meet((uint64_t)(uintptr_t)j->in, (uint64_t)(uintptr_t)j->out, j->in_stride,
                                     rin, rout, j->n_records))
                return NOISE_ERROR_INVALID_PARAM;
        } else if (meet(job_span(j, false, open), job_span(j, true, open))) {
            return NOISE_ERROR_INVALID_PARAM;
        }
    }
    return NOISE_ERROR_NONE;
}

/* does [r.lo, r.hi) reach anything job j writes: its output records, an
   open's statuses */
inline bool range_hits_output(Span r, const NoiseAeadUniform *j, bool open)
{
    if (r.lo == r.hi) return false;
    return meet(r, job_span(j, true, open)) || (open && j->status && meet(r, status_span(j)));
}

/* The jobs of a duplex launch are independent: nothing one job writes
   (records, statuses) may overlap anything the other reads (records, AD) or
   writes. */
inline int check_duplex(const NoiseAeadUniform *sj, const NoiseAeadUniform *oj)
{
    int rc = check_uniform(sj, false);
    if (!rc) rc = check_uniform(oj, true);
    if (rc || !sj->n_records || !oj->n_records) return rc;
    const Span s_in = job_span(sj, false, false), s_out = job_span(sj, true, false);
    const bool clash = meet(s_out, job_span(oj, false, true)) || meet(s_out, job_span(oj, true, true)) ||
                       meet(job_span(oj, true, true), s_in) || range_hits_output(ad_span(oj), sj, false) ||
                       range_hits_output(ad_span(sj), oj, true) || range_hits_output(status_span(oj), sj, false) ||
                       (oj->status && meet(status_span(oj), s_in));
    return clash ? NOISE_ERROR_INVALID_PARAM : NOISE_ERROR_NONE;
}

inline int check_ragged(const NoiseAeadRagged *job)
{
    return (!job || !job->recs || !job->in || !job->out) ? NOISE_ERROR_INVALID_PARAM : NOISE_ERROR_NONE;
}

/* The jobs of a ragged duplex launch are independent too, but their
   descriptors live in device memory: that no record or AD range of one job
   meets anything the other writes is the caller's guarantee (stated in the
   header, not checked, as for the ragged calls).  The host sees the two
   status arrays: they may not meet. */
inline Span ragged_status_span(const NoiseAeadRagged *j)
{
    const u128 lo = (uintptr_t)j->status;
    return {lo, j->status ? lo + j->n_records : lo};
}

inline int check_duplex_ragged(const NoiseAeadRagged *sj, const NoiseAeadRagged *oj)
{
    int rc = check_ragged(sj);
    if (!rc) rc = check_ragged(oj);
    if (rc) return rc;
    const Span s = ragged_status_span(sj), o = ragged_status_span(oj);
    return s.lo != s.hi && o.lo != o.hi && meet(s, o) ? NOISE_ERROR_INVALID_PARAM : NOISE_ERROR_NONE;
}

/* Batched X25519 (noise_aead_dev_dh_calculate / _dh_public; launch_dh.hip).
   The span of n 32-byte keys a stride apart; stride 0 is one key for all. */
inline Span item_span(const void *p, uint64_t stride, uint32_t n, uint32_t item)
{
    const u128 lo = (uintptr_t)p;
    return {lo, lo + (u128)(n - 1) * stride + item};
}

inline Span dh_key_span(const void *p, uint64_t stride, uint32_t n) { return item_span(p, stride, n, 32); }

/* pub == nullptr with has_pub false: the base point (noise_aead_dev_dh_public).
   NOISE_ERROR_NONE with n == 0 means "nothing to do". */
inline int check_dh(int dh_id, const void *priv, uint64_t priv_stride, bool has_pub, const void *pub,
                    uint64_t pub_stride, uint32_t n, const void *out)
{
    if (dh_id != NOISE_DH_CURVE25519) return NOISE_ERROR_UNKNOWN_ID;
    if (!n) return NOISE_ERROR_NONE;
    if (!priv || !out || (has_pub && !pub)) return NOISE_ERROR_INVALID_PARAM;
    if ((priv_stride && priv_stride < 32) || (has_pub && pub_stride && pub_stride < 32))
        return NOISE_ERROR_INVALID_PARAM;
    const Span o = dh_key_span(out, 32, n);
    if (meet(o, dh_key_span(priv, priv_stride, n)) || (has_pub && meet(o, dh_key_span(pub, pub_stride, n))))
        return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* REKEY of n raw 32-byte keys (noise_aead_dev_rekey, header section 12): the
   successors may go exactly where the keys are, and nowhere else that meets
   them.  NOISE_ERROR_NONE with n == 0 means "nothing to do". */
inline int check_rekey(int cipher_id, const void *keys, uint32_t n, const void *out)
{
    if (cipher_id != NOISE_CIPHER_CHACHAPOLY && cipher_id != NOISE_CIPHER_AESGCM) return NOISE_ERROR_UNKNOWN_ID;
    if (!n) return NOISE_ERROR_NONE;
    if (!keys || !out) return NOISE_ERROR_INVALID_PARAM;
    if (out != keys && meet(dh_key_span(out, 32, n), dh_key_span(keys, 32, n))) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* Batched Ed25519 (noise_aead_dev_sign_verify / _sign_public / _sign, header
   section 17; launch_sign.hip).  The rules in the header's order: the id,
   n == 0, the pointers, the strides, then every output range against every
   input the host can see (the message spans are the caller's guarantee). */

inline bool sign_key_stride_bad(uint64_t stride) { return stride && stride < 32; }

/* the offset and length arrays of a ragged message list against an output */
inline bool sign_lists_meet(Span o, const void *off, const void *len, uint32_t n)
{
    return meet(o, item_span(off, 8, n, 8)) || meet(o, item_span(len, 4, n, 4));
}

inline int check_sign_verify(int sign_id, const void *pub, uint64_t pub_stride, const void *sig, uint64_t sig_stride,
                             const void *msg, const void *msg_off, const void *msg_len, uint32_t n,
                             const void *status_in, const void *status)
{
    if (sign_id != NOISE_SIGN_ED25519) return NOISE_ERROR_UNKNOWN_ID;
    if (!n) return NOISE_ERROR_NONE;
    if (!pub || !sig || !msg || !msg_off || !msg_len || !status) return NOISE_ERROR_INVALID_PARAM;
    if (sign_key_stride_bad(pub_stride) || (sig_stride ? sig_stride < 64 : n > 1)) return NOISE_ERROR_INVALID_PARAM;
    const Span o = item_span(status, 1, n, 1);
    if (meet(o, item_span(pub, pub_stride, n, 32)) || meet(o, item_span(sig, sig_stride, n, 64)) ||
        sign_lists_meet(o, msg_off, msg_len, n))
        return NOISE_ERROR_INVALID_PARAM;
    /* in place is the one overlap allowed */
    if (status_in && status_in != status && meet(o, item_span(status_in, 1, n, 1))) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

inline int check_sign_public(int sign_id, const void *priv, uint64_t priv_stride, uint32_t n, const void *pub_out)
{
    if (sign_id != NOISE_SIGN_ED25519) return NOISE_ERROR_UNKNOWN_ID;
    if (!n) return NOISE_ERROR_NONE;
    if (!priv || !pub_out) return NOISE_ERROR_INVALID_PARAM;
    if (sign_key_stride_bad(priv_stride)) return NOISE_ERROR_INVALID_PARAM;
    if (meet(item_span(pub_out, 32, n, 32), item_span(priv, priv_stride, n, 32))) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

inline int check_sign(int sign_id, const void *priv, uint64_t priv_stride, const void *pub, uint64_t pub_stride,
                      const void *msg, const void *msg_off, const void *msg_len, uint32_t n, const void *sig_out)
{
    if (sign_id != NOISE_SIGN_ED25519) return NOISE_ERROR_UNKNOWN_ID;
    if (!n) return NOISE_ERROR_NONE;
    if (!priv || !pub || !msg || !msg_off || !msg_len || !sig_out) return NOISE_ERROR_INVALID_PARAM;
    if (sign_key_stride_bad(priv_stride) || sign_key_stride_bad(pub_stride)) return NOISE_ERROR_INVALID_PARAM;
    const Span o = item_span(sig_out, 64, n, 64);
    if (meet(o, item_span(priv, priv_stride, n, 32)) || meet(o, item_span(pub, pub_stride, n, 32)) ||
        sign_lists_meet(o, msg_off, msg_len, n))
        return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* ------------------------------------------------------ the facts of a job
   FAST layout (chachapoly.hip): 16-B aligned record slots whose input may be
   read up to roundup64(len) — and, for open, holds CT || tag. */
inline bool uniform_fast(const NoiseAeadUniform *j, bool open)
{
    const uint64_t a = (uint64_t)(uintptr_t)j->in | (uint64_t)(uintptr_t)j->out | j->in_stride | j->out_stride;
    if (a & 15) return false;
    const uint64_t need = ((uint64_t)(j->len ? j->len : 1) + 63) & ~63ull;
    if (j->in_stride < need) return false;
    if (open && j->in_stride < (uint64_t)j->len + 16) return false;
    return true;
}

/* lane counts the ChaChaPoly kernels are built for */
inline bool chacha_lanes_ok(uint32_t k) { return k && k <= 64 && !(k & (k - 1)); }

/* ukey: the 64 / k records of every wave share one state (chachapoly.hip
   u_key_nonce), k lanes per record */
inline bool wave_shares_state(uint32_t k, uint32_t recs_per_state) { return recs_per_state % (64u / k) == 0; }

/* the LDS-staged AES-GCM kernels: FAST layout, one state per 256-record
   workgroup */
inline bool gcm_staged_ok(const NoiseAeadUniform *j, bool open)
{
    return uniform_fast(j, open) && j->recs_per_state % PLAN_GCM_WG_RECS == 0;
}

inline bool gcm_lanes_ok(uint32_t lanes_per_record) { return !lanes_per_record || lanes_per_record == PLAN_GCM_LANES; }

/* The open order of a job: verify first — the reference's order
   (cipher-chachapoly.c:135-141, cipher-aesgcm.c:172-188) — for every open
   unless a ChaChaPoly job opts into NOISE_AEAD_FLAG_ONE_PASS (round 6,
   VERDICT r5 item 1; the one-pass order was the ChaChaPoly default through
   round 5, DESIGN.md 4.1b gives the cost).  AES-GCM opens always verify
   first: there it costs nothing (C3 732 vs 726 GiB/s, the C5 AES-GCM open
   0.77 vs 0.82 ms: the GHASH-only pass, then CTR for the verified records,
   profiles/r04_round/).  VERIFY_FIRST overrides ONE_PASS. */
inline bool open_vf(int cipher_id, uint32_t flags, bool open)
{
    const bool flags_vf = (flags & NOISE_AEAD_FLAG_VERIFY_FIRST) || !(flags & NOISE_AEAD_FLAG_ONE_PASS);
    return open && (flags_vf || cipher_id == NOISE_CIPHER_AESGCM);
}

inline bool ct_ghash(uint32_t flags, const Switches &sw) { return (flags & NOISE_AEAD_FLAG_CT_GHASH) || sw.ct_ghash; }

/* ------------------------------------------------------- lanes per record
   ChaChaPoly: 4 (the fastest split at 64 Ki and 1 Mi records,
   profiles/r01_sweep_*), 8 when the batch is too small to give every SIMD
   four waves that way. */
constexpr uint64_t LANES_TARGET = 256ull * 16 * 64; /* 4 waves on each of 1024 SIMDs */

inline int throughput_lanes(uint32_t n_records) { return (uint64_t)n_records * 4 < LANES_TARGET ? 8 : 4; }

/* Batches of at most WIDE_MAX_RECORDS — the single-call latency path, where
   a long record's blocks would otherwise run serially on a few lanes — get
   wider groups, up to one wave per record, but no wider than the longest
   record needs (two ChaCha blocks per lane; max_len = 0 when unknown).
   Larger pipelined chunks (≈ 3 K records of 1400 B) measured faster at 8
   (profiles/r01_hostpaths_ab). */
constexpr uint32_t WIDE_MAX_RECORDS = 512;

inline int auto_lanes(uint32_t n_records, uint32_t max_len)
{
    if (n_records > WIDE_MAX_RECORDS) return throughput_lanes(n_records);
    int k = 4;
    while (k < 64 && (uint64_t)n_records * k < LANES_TARGET) k <<= 1;
    if (max_len) {
        const uint32_t blocks = (max_len + 63) / 64 + 1;
        int need = 4;
        while (need < 64 && (uint32_t)need * 2 < blocks) need <<= 1;
        if (k > need) k = need;
    }
    return k;
}

/* One lane per record (chachapoly.hip seal_solo_staged) for the duplex
   launch of two uniform FAST jobs of at least SOLO_MIN_RECORDS each: one
   Poly1305 chain per record with the clamped r, the per-record work paid
   once per 64 records, and a seal and an open wave on every SIMD; C2
   +8-17 %, C4 +13-18 % over four lanes (profiles/r04/solo_ab.jsonl,
   solo_prio_ab.jsonl).  A standalone seal or open takes one lane from
   SOLO_MIN_STANDALONE records, two waves per SIMD: C4's 1 Mi records as
   back-to-back seal and open launches 1624-1636 vs 1410-1415 GiB/s at four
   lanes, while a 64 Ki-record job alone (one wave per SIMD) runs 3 % faster
   at four lanes (1315-1321 vs 1280-1283, profiles/r04/separate_lanes_ab.jsonl);
   a verify-first open (the default) too since round 6's 4/8-lane
   verify-first staged kernel (chachapoly.hip open_il_staged_vf): 1388-1389
   vs 1236-1262 GiB/s at 64 Ki x 1400 B (profiles/r06/vf_staged_ab/).
   lanes_per_record = 2 on a FAST layout always takes the two-segment kernel. */
constexpr uint32_t SOLO_MIN_RECORDS = 65536;
constexpr uint32_t SOLO_MIN_STANDALONE = 2 * SOLO_MIN_RECORDS;

/* fast: the job's layout is FAST; duplex: it is one job of a duplex launch */
inline int chacha_uniform_lanes(uint32_t lanes_per_record, uint32_t n_records, bool fast, bool duplex,
                                const Switches &sw)
{
    if (lanes_per_record) return (int)lanes_per_record;
    if (n_records >= SOLO_MIN_RECORDS && sw.solo && fast) {
        if (duplex || n_records >= SOLO_MIN_STANDALONE) return 1;
        if (sw.seg == 2) return 2;
    }
    return auto_lanes(n_records, 0);
}

/* ragged records are often long (C5 mixes 64 B-16 KiB): 8 lanes up to
   128 Ki records, two generations of waves that even out the mixed lengths
   (C5's ChaCha kernels -2.5 % seal / -4 % open at 64 Ki records vs 4 lanes,
   profiles/r02/c5_lanes_ab.jsonl) */
inline int chacha_ragged_lanes(uint32_t lanes_per_record, uint32_t n_records)
{
    if (lanes_per_record) return (int)lanes_per_record;
    const int k = auto_lanes(n_records, 0);
    return k == 4 && n_records < SOLO_MIN_STANDALONE ? 8 : k;
}

/* the host paths (cipherstate.c, wire.c) know their records' lengths */
inline uint32_t host_chacha_lanes(uint32_t n_records, uint32_t max_len, const Switches &sw)
{
    if (sw.lanes_narrow) return (uint32_t)throughput_lanes(n_records);
    return (uint32_t)auto_lanes(n_records, max_len ? max_len : 1);
}

/* 0: automatic (a small ragged batch runs a workgroup per record) */
inline uint32_t host_aes_lanes(const Switches &sw) { return sw.lanes_narrow ? PLAN_GCM_LANES : 0; }

/* Ragged FAST ChaChaPoly batches of at least SEG_RAGGED_MIN records with
   automatic lanes take the segmented one-lane kernel (a per-launch plan by
   record length, chachapoly_seg.hip); smaller ones keep the windowed 4/8-lane
   kernels and the wide groups of the latency path.  The plan packs
   record << 6 | segment into 32 bits (chachapoly_seg.hip seg_plan_place) and
   counts lanes in 32 bits: batches of 2^26 records or more keep the windowed
   kernels. */
constexpr uint32_t SEG_RAGGED_MIN = 16384;
constexpr uint32_t SEG_RAGGED_MAX = 1u << 26;

inline bool ragged_takes_seg(int cipher_id, const NoiseAeadRagged *job, const Switches &sw)
{
    return cipher_id == NOISE_CIPHER_CHACHAPOLY && !job->lanes_per_record && (job->flags & NOISE_AEAD_FLAG_FAST) &&
           job->n_records >= SEG_RAGGED_MIN && job->n_records < SEG_RAGGED_MAX && sw.seg != 0;
}

/* ---------------------------------------------------------------- the plan
   One value per kernel family; the Plan's fields hold its template
   arguments (plan_print names which). */
enum Kernel : uint8_t {
    K_NONE,
    K_CHACHA_UNIFORM,       /* chachapoly_{seal,open}_uniform<K, FAST> */
    K_CHACHA_STAGED,        /* chachapoly_{seal,open}_staged<K, UKEY>, K = 4, 8 */
    K_CHACHA_STAGED_VF,     /* chachapoly_open_staged_vf<K, UKEY> */
    K_CHACHA_SOLO,          /* chachapoly_{seal,open}_solo<UKEY, RUNS> */
    K_CHACHA_SEG2,          /* chachapoly_seg2_uniform<OPEN, UKEY> */
    K_CHACHA_DUPLEX_SOLO,   /* chachapoly_duplex_solo<UKEY> */
    K_CHACHA_DUPLEX_STAGED, /* chachapoly_duplex_staged<K, UKEY> */
    K_CHACHA_RAGGED,        /* chachapoly_seal_ragged<K, FAST>, chachapoly_open_ragged<K, FAST[, VF]> */
    K_CHACHA_SEG_RAGGED,    /* chachapoly_seg_ragged<OPEN> */
    K_CHACHA_DUPLEX_RAGGED, /* chachapoly_duplex_ragged<K, FAST, VF> */
    K_CHACHA_SEG_DUPLEX,    /* chachapoly_seg_duplex */
    K_GCM_UNIFORM,          /* gcm_uniform<OPEN, CT> */
    K_GCM_STAGED,           /* gcm_staged<OPEN, CT> */
    K_GCM_DUPLEX_FUSED,     /* gcm_duplex_fused<CT> */
    K_GCM_DUPLEX_STAGED,    /* gcm_duplex_staged<CT> */
    K_GCM_WIDE,             /* gcm_wide<OPEN, CT> */
    K_GCM_RAGGED,           /* gcm_ragged_staged<OPEN, FAST, WG, CT, R, KL> */
    K_GCM_DUPLEX_RAGGED,    /* gcm_duplex_ragged<FAST, WG, CT, R, KL> */
};

struct Plan {
    int rc = NOISE_ERROR_NONE; /* not NONE: the job is refused, nothing else is set */
    Kernel kernel = K_NONE;
    bool shared = false;       /* plan_duplex, plan_duplex_ragged: the two jobs share this launch; else plan each alone */
    /* template arguments */
    bool open = false, fast = false, ukey = false, runs = false, vf_order = false, ct = false;
    int wg = 0, r = 0;         /* gcm_ragged_staged: threads per workgroup, records per group */
    int lanes = 0;             /* lanes per record: K, KL */
    /* launch */
    uint32_t grid = 0;         /* 0: an empty job, nothing to launch */
    uint32_t block = PLAN_BLOCK;
    uint32_t park = 0;         /* worker_park_for_batch's workgroup count (0: not asked) */
    /* kernel arguments */
    uint32_t sb = 0, ob = 0;   /* duplex: the seal and the open job's workgroups */
    uint32_t balance = 0;      /* UniformArgs::balance of every job of the launch */
    uint32_t vf = 0;           /* UniformArgs / RaggedArgs::vf of the open job */
    uint32_t run = 0;          /* chachapoly_duplex_solo's run length */
};

inline Plan refused(int rc)
{
    Plan p;
    p.rc = rc;
    return p;
}

inline bool plan_is_gcm(const Plan &p) { return p.kernel >= K_GCM_UNIFORM; }

inline uint32_t blocks_for(uint64_t items, uint32_t per_block) { return (uint32_t)((items + per_block - 1) / per_block); }

/* balance: the launch is one resident generation of waves, so the kernel
   balances their progress (aead_device.h prio_by_progress; open:
   profiles/r01_prio_ab.jsonl; seal: +3-8 % once the key stream ran in runs,
   chachapoly.hip slot_block).  The 4-waves-per-SIMD kernels (NA_UNIFORM_OCC)
   count with 1024 resident workgroups, the one-lane kernels (two 64-record
   waves per SIMD at most, chachapoly.hip solo_blocks2) with two per CU of
   the device at hand.  chachapoly_duplex_staged does not read it. */
inline uint32_t balance_of(Kernel kernel, uint32_t grid, uint32_t cus)
{
    if (kernel == K_CHACHA_DUPLEX_STAGED) return 0;
    const bool one_lane = kernel == K_CHACHA_SOLO || kernel == K_CHACHA_DUPLEX_SOLO;
    return grid <= (one_lane ? 2 * (uint64_t)cus : 1024u);
}

/* A uniform seal or open.  cus: the device's CU count (0: unknown). */
inline Plan plan_uniform(int cipher_id, const NoiseAeadUniform *j, bool open, const Switches &sw, uint32_t cus)
{
    Plan p;
    p.open = open;
    p.fast = uniform_fast(j, open);
    p.vf = open_vf(cipher_id, j->flags, open);
    if (cipher_id == NOISE_CIPHER_CHACHAPOLY) {
        const uint32_t k = (uint32_t)chacha_uniform_lanes(j->lanes_per_record, j->n_records, p.fast, false, sw);
        if (!chacha_lanes_ok(k)) return refused(NOISE_ERROR_INVALID_PARAM);
        p.lanes = (int)k;
        p.ukey = wave_shares_state(k, j->recs_per_state);
        if (!p.fast || k > 8) {
            p.kernel = K_CHACHA_UNIFORM;
        } else if (k == 1) {
            /* the key stream issued in runs once the launch is two waves per
               SIMD (64 records per wave, four SIMDs per CU) */
            p.kernel = K_CHACHA_SOLO;
            p.runs = cus && j->n_records >= 2ull * 4 * 64 * cus;
        } else if (k == 2) {
            p.kernel = K_CHACHA_SEG2; /* two segments per record, LDS-staged */
        } else {
            /* a verify-first open takes an AUTH + DEC kernel, never the
               one-pass staged ones */
            p.kernel = p.vf ? K_CHACHA_STAGED_VF : K_CHACHA_STAGED;
        }
        p.grid = p.park = blocks_for((uint64_t)j->n_records * k, PLAN_BLOCK);
        p.balance = balance_of(p.kernel, p.grid, cus);
        return p;
    }
    if (cipher_id == NOISE_CIPHER_AESGCM) {
        if (!gcm_lanes_ok(j->lanes_per_record)) return refused(NOISE_ERROR_INVALID_PARAM);
        p.lanes = (int)PLAN_GCM_LANES;
        p.ct = ct_ghash(j->flags, sw);
        if (gcm_staged_ok(j, open)) {
            p.kernel = K_GCM_STAGED;
            p.block = PLAN_GCM_WG;
            p.grid = p.park = blocks_for(j->n_records, PLAN_GCM_WG_RECS);
        } else {
            p.kernel = K_GCM_UNIFORM;
            p.grid = p.park = blocks_for((uint64_t)j->n_records * PLAN_GCM_LANES, PLAN_BLOCK);
        }
        return p;
    }
    return refused(NOISE_ERROR_UNKNOWN_ID);
}

/* A duplex of two checked jobs: one launch (shared) when both jobs take the
   same kernel family, else each job is planned alone (plan_uniform).  A
   verify-first open shares a launch only with kernels that run its order:
   the one-lane ChaChaPoly open (AUTH + DEC passes) and the staged AES-GCM
   open (GHASH, verdict, then CTR). */
inline Plan plan_duplex(int cipher_id, const NoiseAeadUniform *sj, const NoiseAeadUniform *oj, const Switches &sw,
                        uint32_t cus)
{
    Plan p;
    if (!sj->n_records || !oj->n_records || !uniform_fast(sj, false) || !uniform_fast(oj, true)) return p;
    p.fast = true;
    p.vf = open_vf(cipher_id, oj->flags, true);
    if (cipher_id == NOISE_CIPHER_CHACHAPOLY) {
        const uint32_t k = (uint32_t)chacha_uniform_lanes(sj->lanes_per_record, sj->n_records, true, true, sw);
        if (k != (uint32_t)chacha_uniform_lanes(oj->lanes_per_record, oj->n_records, true, true, sw)) return p;
        if (!(k == 1 || ((k == 4 || k == 8) && !p.vf))) return p;
        p.ukey = wave_shares_state(k, sj->recs_per_state);
        if (p.ukey != wave_shares_state(k, oj->recs_per_state)) return p;
        p.shared = true;
        p.lanes = (int)k;
        p.kernel = k == 1 ? K_CHACHA_DUPLEX_SOLO : K_CHACHA_DUPLEX_STAGED;
        p.sb = blocks_for((uint64_t)sj->n_records * k, PLAN_BLOCK);
        p.ob = blocks_for((uint64_t)oj->n_records * k, PLAN_BLOCK);
        p.grid = p.park = p.sb + p.ob;
        p.balance = balance_of(p.kernel, p.grid, cus);
        /* one seal and one open block per CU */
        if (k == 1) p.run = sw.duplex_runs ? cus : 0;
        return p;
    }
    if (cipher_id == NOISE_CIPHER_AESGCM) {
        if (!gcm_lanes_ok(sj->lanes_per_record) || !gcm_lanes_ok(oj->lanes_per_record)) return p;
        if (!gcm_staged_ok(sj, false) || !gcm_staged_ok(oj, true)) return p;
        p.ct = ct_ghash(sj->flags, sw);
        if (p.ct != ct_ghash(oj->flags, sw)) return p;
        p.shared = true;
        p.lanes = (int)PLAN_GCM_LANES;
        p.block = PLAN_GCM_WG;
        p.sb = blocks_for(sj->n_records, PLAN_GCM_WG_RECS);
        p.ob = blocks_for(oj->n_records, PLAN_GCM_WG_RECS);
        p.park = p.sb > p.ob ? p.sb : p.ob;
        p.kernel = sw.gcm_duplex_fused ? K_GCM_DUPLEX_FUSED : K_GCM_DUPLEX_STAGED;
        p.grid = sw.gcm_duplex_fused ? p.park : p.sb + p.ob;
        return p;
    }
    return p;
}

/* Ragged AES-GCM launch shape: threads per workgroup, records per group
   and lanes per record (gcm_ragged_staged).  A workgroup owns its CU (the
   LDS T-tables), so its time is its longest wave's; pairing a long with a
   short record per group (R = 2) evens the waves out: +21 % records per
   CU-second on C5's 64 B-16 KiB mix (profiles/r02/c5_gcm_shape_ab.jsonl).
   From 131072 records on every CU gets a 512-record window of 4-lane groups;
   from 65536 on, 256-record windows of 8-lane groups (KL = 8, H^8 Horner)
   keep all CUs busy with the same pairing (4-lane pairs there would idle
   half the CUs: 1.55 vs 0.94 ms); smaller batches take 256-thread
   workgroups over 64-record windows (4x the workgroups). */
struct GcmShape { int wg, r, kl; };

inline GcmShape gcm_ragged_shape(uint32_t n, const Switches &sw)
{
    if (sw.gcm_shape == 1) return {1024, 1, 4};
    if (sw.gcm_shape == 2) return {1024, 2, 4};
    if (sw.gcm_shape == 3) return {1024, 2, 8};
    if (n >= 256u * 2 * PLAN_GCM_WG_RECS) return {1024, 2, 4};
    if (n >= 256u * PLAN_GCM_WG_RECS) return {1024, 2, 8};
    return {256, 1, 4};
}

/* A ragged seal or open.  seg_resident: resident workgroups of the
   segmented kernel on the device, asked only when ragged_takes_seg(). */
inline Plan plan_ragged(int cipher_id, const NoiseAeadRagged *j, bool open, const Switches &sw, uint32_t seg_resident)
{
    Plan p;
    const uint32_t n = j->n_records;
    p.open = open;
    p.fast = (j->flags & NOISE_AEAD_FLAG_FAST) != 0;
    p.vf = open_vf(cipher_id, j->flags, open);
    if (cipher_id == NOISE_CIPHER_CHACHAPOLY) {
        if (ragged_takes_seg(cipher_id, j, sw)) {
            /* a persistent grid: the resident workgroups, or fewer when the
               batch cannot fill them (jobs / 4, at most) */
            if (!seg_resident) return refused(NOISE_ERROR_SYSTEM);
            const uint32_t most = blocks_for((uint64_t)n * PLAN_SEG_KMAX, PLAN_BLOCK);
            p.kernel = K_CHACHA_SEG_RAGGED;
            p.lanes = 1;
            p.grid = p.park = most > seg_resident ? seg_resident : most;
            return p;
        }
        const uint32_t k = (uint32_t)chacha_ragged_lanes(j->lanes_per_record, n);
        if (!chacha_lanes_ok(k)) return refused(NOISE_ERROR_INVALID_PARAM);
        p.kernel = K_CHACHA_RAGGED;
        p.lanes = (int)k;
        /* the FAST opens' two-pass (verify-first) instantiation; the generic
           layouts' opens and the 1- and 2-lane ones are two-pass already */
        p.vf_order = open && p.fast && p.vf && k >= 4;
        p.grid = p.park = blocks_for((uint64_t)n * k, PLAN_BLOCK);
        return p;
    }
    if (cipher_id == NOISE_CIPHER_AESGCM) {
        p.ct = ct_ghash(j->flags, sw);
        if (!j->lanes_per_record && n <= WIDE_MAX_RECORDS) {
            /* small batch with automatic lanes: a workgroup per record
               (latency, not throughput); lanes_per_record = 4 keeps the
               windowed 4-lane kernels */
            p.kernel = K_GCM_WIDE;
            p.lanes = (int)PLAN_BLOCK;
            p.grid = n;
            return p;
        }
        const GcmShape sh = gcm_ragged_shape(n, sw);
        p.kernel = K_GCM_RAGGED;
        p.wg = sh.wg, p.r = sh.r, p.lanes = sh.kl;
        p.block = (uint32_t)p.wg;
        p.grid = p.park = blocks_for(n, (uint32_t)(p.wg / p.lanes * p.r)); /* records per window */
        return p;
    }
    return refused(NOISE_ERROR_UNKNOWN_ID);
}

/* Which families' shared ragged launch noise_aead_dev_duplex_ragged takes
   when NOISE_AEAD_RAGGED_DUPLEX is unset: the ones measured faster than the
   better of the two separate launches (one stream, two streams) by more
   than the spread between repeats of one arm, on C5's data with two sets
   (tools/duplex_ragged_ab.py, profiles/duplex_ragged_ab.jsonl, DESIGN.md
   4.9).  A family that is off stays built, tested and reachable with
   NOISE_AEAD_RAGGED_DUPLEX=1.  vf: the open job verifies first.
   - chachapoly_seg_duplex: 700.6 vs 753.4 us per step (-7.0 %, spread
     <= 2.9 %) with a one-pass open: on; with a verify-first open 803.7 vs
     809.9 us (-0.8 %, spread <= 1.4 %): off;
   - gcm_duplex_ragged<.., 2, 8>: 1544.1 vs 1439.9 us (+7.2 %): off;
   - chachapoly_duplex_ragged<8, true, true> (the same data under
     NOISE_AEAD_SEG=0): 985.3 vs 890.4 us (+10.7 %): off. */
inline bool ragged_duplex_default(Kernel k, bool vf)
{
    switch (k) {
    case K_CHACHA_SEG_DUPLEX: return !vf;
    case K_CHACHA_DUPLEX_RAGGED:
    case K_GCM_DUPLEX_RAGGED:
    default: return false;
    }
}

/* A ragged duplex of two checked jobs: one launch (shared) when both jobs
   take, each planned alone (plan_ragged), the same kernel family with the
   same template arguments — a job in a shared launch runs exactly what it
   would run alone.  Else (shared = false) each job is planned and launched
   alone, seal first.  A job that plan_ragged refuses is refused here with
   the same rc (the seal job's first).  seg_resident: resident workgroups of
   the kernel the segmented jobs would run (chachapoly_seg_duplex when both
   are segmented). */
inline Plan plan_duplex_ragged(int cipher_id, const NoiseAeadRagged *sj, const NoiseAeadRagged *oj,
                               const Switches &sw, uint32_t seg_resident)
{
    const Plan ps = plan_ragged(cipher_id, sj, false, sw, seg_resident);
    if (ps.rc) return refused(ps.rc);
    const Plan po = plan_ragged(cipher_id, oj, true, sw, seg_resident);
    if (po.rc) return refused(po.rc);
    Plan p;
    if (!sj->n_records || !oj->n_records || sw.ragged_duplex == 0 || ps.kernel != po.kernel) return p;
    if (ps.kernel == K_CHACHA_SEG_RAGGED) {
        /* one ticket over both plans' jobs on the persistent grid */
        const uint64_t most = (uint64_t)blocks_for((uint64_t)sj->n_records * PLAN_SEG_KMAX, PLAN_BLOCK) +
                              blocks_for((uint64_t)oj->n_records * PLAN_SEG_KMAX, PLAN_BLOCK);
        p.kernel = K_CHACHA_SEG_DUPLEX;
        p.lanes = 1;
        p.grid = p.park = most > seg_resident ? seg_resident : (uint32_t)most;
        p.sb = ps.grid, p.ob = po.grid;
    } else if (ps.kernel == K_CHACHA_RAGGED) {
        if (ps.lanes != po.lanes || ps.fast != po.fast) return p;
        if ((uint64_t)ps.grid + po.grid > 0xFFFFFFFFull) return p;
        p.kernel = K_CHACHA_DUPLEX_RAGGED;
        p.lanes = ps.lanes;
        p.vf_order = po.vf_order;
        p.sb = ps.grid, p.ob = po.grid;
        p.grid = p.park = p.sb + p.ob;
    } else if (ps.kernel == K_GCM_RAGGED) {
        if (ps.wg != po.wg || ps.r != po.r || ps.lanes != po.lanes || ps.fast != po.fast || ps.ct != po.ct) return p;
        p.kernel = K_GCM_DUPLEX_RAGGED;
        p.wg = ps.wg, p.r = ps.r, p.lanes = ps.lanes;
        p.ct = ps.ct;
        p.block = ps.block;
        p.sb = ps.grid, p.ob = po.grid;
        p.grid = p.park = p.sb > p.ob ? p.sb : p.ob;
    } else {
        return p; /* gcm_wide: a workgroup per record, nothing to share */
    }
    if (sw.ragged_duplex < 0 && !ragged_duplex_default(p.kernel, po.vf)) return Plan();
    p.shared = true;
    p.fast = ps.fast;
    p.vf = po.vf;
    return p;
}

/* The printed form of a plan: the kernel as its symbol demangles (without
   namespace and arguments), then the launch and the kernel arguments.  The
   golden plan table and noise_aead_debug_last_plan share it. */
inline int plan_print(const Plan &p, char *buf, size_t size)
{
    const char *b[2] = {"false", "true"};
    const char *so = p.open ? "open" : "seal";
    char name[96];
    switch (p.kernel) {
    case K_NONE: snprintf(name, sizeof name, "none"); break;
    case K_CHACHA_UNIFORM: snprintf(name, sizeof name, "chachapoly_%s_uniform<%d,%s>", so, p.lanes, b[p.fast]); break;
    case K_CHACHA_STAGED: snprintf(name, sizeof name, "chachapoly_%s_staged<%d,%s>", so, p.lanes, b[p.ukey]); break;
    case K_CHACHA_STAGED_VF: snprintf(name, sizeof name, "chachapoly_open_staged_vf<%d,%s>", p.lanes, b[p.ukey]); break;
    case K_CHACHA_SOLO: snprintf(name, sizeof name, "chachapoly_%s_solo<%s,%s>", so, b[p.ukey], b[p.runs]); break;
    case K_CHACHA_SEG2: snprintf(name, sizeof name, "chachapoly_seg2_uniform<%s,%s>", b[p.open], b[p.ukey]); break;
    case K_CHACHA_DUPLEX_SOLO: snprintf(name, sizeof name, "chachapoly_duplex_solo<%s>", b[p.ukey]); break;
    case K_CHACHA_DUPLEX_STAGED: snprintf(name, sizeof name, "chachapoly_duplex_staged<%d,%s>", p.lanes, b[p.ukey]); break;
    case K_CHACHA_RAGGED:
        if (p.open) snprintf(name, sizeof name, "chachapoly_open_ragged<%d,%s,%s>", p.lanes, b[p.fast], b[p.vf_order]);
        else snprintf(name, sizeof name, "chachapoly_seal_ragged<%d,%s>", p.lanes, b[p.fast]);
        break;
    case K_CHACHA_SEG_RAGGED: snprintf(name, sizeof name, "chachapoly_seg_ragged<%s>", b[p.open]); break;
    case K_CHACHA_DUPLEX_RAGGED:
        snprintf(name, sizeof name, "chachapoly_duplex_ragged<%d,%s,%s>", p.lanes, b[p.fast], b[p.vf_order]);
        break;
    case K_CHACHA_SEG_DUPLEX: snprintf(name, sizeof name, "chachapoly_seg_duplex"); break;
    case K_GCM_UNIFORM: snprintf(name, sizeof name, "gcm_uniform<%s,%s>", b[p.open], b[p.ct]); break;
    case K_GCM_STAGED: snprintf(name, sizeof name, "gcm_staged<%s,%s>", b[p.open], b[p.ct]); break;
    case K_GCM_DUPLEX_FUSED: snprintf(name, sizeof name, "gcm_duplex_fused<%s>", b[p.ct]); break;
    case K_GCM_DUPLEX_STAGED: snprintf(name, sizeof name, "gcm_duplex_staged<%s>", b[p.ct]); break;
    case K_GCM_WIDE: snprintf(name, sizeof name, "gcm_wide<%s,%s>", b[p.open], b[p.ct]); break;
    case K_GCM_RAGGED:
        snprintf(name, sizeof name, "gcm_ragged_staged<%s,%s,%d,%s,%d,%d>", b[p.open], b[p.fast], p.wg, b[p.ct], p.r,
                 p.lanes);
        break;
    case K_GCM_DUPLEX_RAGGED:
        snprintf(name, sizeof name, "gcm_duplex_ragged<%s,%d,%s,%d,%d>", b[p.fast], p.wg, b[p.ct], p.r, p.lanes);
        break;
    }
    if (p.sb || p.ob)
        return snprintf(buf, size, "%s grid=%u block=%u park=%u bal=%u/%u vf=0/%u sb=%u ob=%u run=%u", name, p.grid,
                        p.block, p.park, p.balance, p.balance, p.vf, p.sb, p.ob, p.run);
    return snprintf(buf, size, "%s grid=%u block=%u park=%u bal=%u vf=%u", name, p.grid, p.block, p.park, p.balance,
                    p.vf);
}

} // namespace na
