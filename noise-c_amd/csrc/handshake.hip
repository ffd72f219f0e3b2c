/*
 * handshake.hip — batched Noise handshakes on the device:
 * noise_aead_dev_handshake_* (include/noise_aead_hip.h section 8).
 *
 * The host object walks the steps handshake_plan.h makes of a message and
 * issues, per step, launches over all n sessions; nothing comes back to the
 * host, so the action, the nonce and "is a key set" — which are the same for
 * every session of a batch — live on the host and everything per session
 * (ck, h, k, statuses, public keys) lives on the device, in one DevArena
 * (launch.h): zeroed before use, zeroed again before it is freed.
 *
 * The kernels here run one lane per session in 64-lane workgroups
 * (launch_items, launch.h) over the SymmetricState arithmetic of hasher.h —
 * kdf_hkdf, kdf_mix_hash, load_row / store_row for a session's h or ck; none
 * of it is restated here:
 *   hs_init       h = the protocol name padded or hashed, ck = h
 *                 (symmetricstate.c:97-108);
 *   hs_mix_hash   h = HASH(h || bytes), with an optional copy of the bytes (the
 *                 pass-through of an unkeyed encrypt/decrypt_and_hash, an `e`
 *                 into or out of a message), and, after an open, the sticky
 *                 status merge: a session whose tag failed keeps its h and
 *                 takes status 1.  Session i's bytes lie i * stride from the
 *                 base or at a per-session offset (HsRows) and have a fixed
 *                 or a per-session length (HsLens): the uniform and the
 *                 ragged message calls run this one body.  As the payload
 *                 step of a ragged call it also writes the out-length array;
 *   hs_check_len  the front step of a ragged call: a session whose length
 *                 hs_session_len (handshake_plan.h) refuses takes status 4
 *                 before any token;
 *   hs_mix_key    ck, k = HKDF(ck, ikm) in place, zeroing the shared secret
 *                 it consumed (noise_clean(shared), handshakestate.c:1136);
 *                 for the PSK start-up step ck, temp = HKDF(ck, psk) and
 *                 MixHash(temp) (:833-842);
 *   hs_null_check the all-zero received ephemeral (:1464-1470) -> status 3;
 *   hs_build_recs the NoiseAeadRecord array of one AEAD step from (rows,
 *                 lengths, nonce, i * ctx_bytes, i * hash_len); a failed
 *                 session gets the length the ragged kernels refuse (REFUSED_LEN,
 *                 aead_kernels.h), so nothing more is sealed or opened for it;
 *   hs_split      k1, k2 = HKDF(ck, ""), zeros for a failed session, and h;
 *   hs_fallback_take   the Noise Pipes fallback (header section 15): which
 *                 sessions of a handshake go on in the XXfallback object made of
 *                 it (hs_fallback_takes, handshake_plan.h) — status 0 there, 5
 *                 for the others, 5 here for a live session that leaves — and
 *                 the copy of the public keys the new object keeps;
 *   hs_fallback_merge  the fallback's split folded into the original's, the
 *                 keys swapped back into the original role's orientation;
 *   hs_move       sessions that change their object (header section 16): entry
 *                 j of a lane list by hs_move_rule (handshake_plan.h) — a moved
 *                 session's ck, h, k, status, keys received and per-session key
 *                 rows go through registers into the other object's lane, then
 *                 the lane it left is scrubbed;
 *   hs_drop       that scrub alone: the lane's rows zeroed, its status 5.
 * A fallback object is an ordinary object whose pattern is HS_XXFALLBACK: its
 * start-up ends with the pre-message e, and every call below serves it.
 * DH tokens are the ladder launches of noise_aead_dev_dh_calculate into an
 * arena the object owns; the AEAD steps are noise_aead_dev_seal_ragged /
 * _open_ragged (verify-first) under AD = h; AES-GCM key contexts are prepared
 * again only when k changed since the last prepare (ChaChaPoly's context is
 * the key itself).
 */
#include "launch.h"

#include "handshake_plan.h"
#include "hasher.h"

#include <new>

using namespace na;

namespace {

constexpr uint32_t HS_BLOCK = 64;
constexpr size_t HS_ALIGN = 64; /* of the parts of the object's device allocation */
constexpr uint8_t HS_STATUS_MAC = 1, HS_STATUS_NULL_KEY = 3;

struct InitArgs {
    int hash_id;
    uint32_t hl, n, name_len;
    uint8_t *h, *ck;
    uint8_t name[HS_NAME_MAX];
};

__global__ __launch_bounds__(HS_BLOCK) void hs_init(InitArgs a)
{
    const uint32_t i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    uint8_t h[64];
    if (a.name_len <= a.hl) {
        for (uint32_t j = 0; j < a.hl; ++j) h[j] = j < a.name_len ? a.name[j] : 0;
    } else {
        Hasher H;
        H.init(a.hash_id);
        H.update(a.name, a.name_len);
        H.final(h);
    }
    for (uint32_t j = 0; j < a.hl; ++j) a.h[(size_t)i * a.hl + j] = a.ck[(size_t)i * a.hl + j] = h[j]; /* one pass, two rows */
}

/* Where session i's bytes lie from a base pointer: i * stride (0: one value
   for all), or off[i] — any order, any alignment.  The ragged calls put the
   token's offset inside the message into the base pointer. */
struct HsRows {
    const uint64_t *off;
    uint64_t stride;
    __device__ __forceinline__ uint64_t at(uint32_t i) const { return off ? off[i] : (uint64_t)i * stride; }
};

/* Session i's length in a step: `fixed` (a key token, a uniform call), or
   from the per-session array of a ragged call through hs_session_len
   (handshake_plan.h), the one statement of the length rule. */
struct HsLens {
    const uint32_t *per; /* write: payload lengths; read: message lengths */
    uint32_t fixed, overhead, write;
    __device__ __forceinline__ bool refused(uint32_t i) const
    {
        return hs_session_len(overhead, per ? per[i] : fixed, write).refused;
    }
    __device__ __forceinline__ uint32_t payload(uint32_t i) const
    {
        if (!per) return fixed;
        return write ? per[i] : hs_session_len(overhead, per[i], false).other;
    }
    /* what the call reports: the message length of a write, the payload length of a read */
    __device__ __forceinline__ uint32_t reported(uint32_t i) const
    {
        const uint32_t p = payload(i);
        return write ? hs_session_len(overhead, p, true).other : p;
    }
};

struct MixHashArgs {
    int hash_id;
    uint32_t hl, n;
    uint8_t *h;
    const uint8_t *src;   /* session i hashes src + src_rows.at(i), lens.payload(i) + extra bytes */
    HsRows src_rows;
    uint8_t *dst;         /* not NULL: the bytes are also copied to dst + dst_rows.at(i) */
    HsRows dst_rows;
    HsLens lens;
    uint32_t extra;       /* the tag after a sealed or opened payload */
    uint8_t *status;      /* the sticky statuses: a failed session does nothing */
    const uint8_t *step;  /* not NULL: the statuses of the open just done */
    uint32_t *out_len;    /* not NULL (the payload step of a ragged call): lens.reported(i), 0 for a failed session */
};

__global__ __launch_bounds__(HS_BLOCK) void hs_mix_hash(MixHashArgs a)
{
    const uint32_t i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    uint8_t st = a.status[i];
    if (!st && a.step && a.step[i]) /* the reference leaves h as it was (symmetricstate.c:436-443) */
        a.status[i] = st = HS_STATUS_MAC;
    if (st) {
        if (a.out_len) a.out_len[i] = 0;
        return;
    }
    const uint32_t len = a.lens.payload(i) + a.extra;
    const uint8_t *src = a.src + a.src_rows.at(i);
    if (a.dst) {
        uint8_t *dst = a.dst + a.dst_rows.at(i);
        for (uint32_t j = 0; j < len; ++j) dst[j] = src[j];
    }
    uint8_t h[64];
    load_row(h, a.h, i, a.hl);
    kdf_mix_hash(a.hash_id, a.hl, h, src, len);
    store_row(a.h, i, a.hl, h);
    if (a.out_len) a.out_len[i] = a.lens.reported(i);
}

/* the front step of a ragged call: the length rule before any token */
__global__ __launch_bounds__(HS_BLOCK) void hs_check_len(HsLens lens, uint8_t *status, uint32_t n)
{
    const uint32_t i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= n || status[i]) return;
    if (lens.refused(i)) status[i] = HS_STATUS_LENGTH;
}

struct MixKeyArgs {
    int hash_id;
    uint32_t hl, n;
    uint8_t *ck, *k;
    uint8_t *h;           /* psk: MixHash(temp) instead of k = temp */
    uint8_t *ikm;         /* 32 bytes at ikm + i * ikm_stride */
    uint64_t ikm_stride;
    uint32_t zero_ikm, psk;
};

__global__ __launch_bounds__(HS_BLOCK) void hs_mix_key(MixKeyArgs a)
{
    const uint32_t i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    uint8_t *ikm_p = a.ikm + (uint64_t)i * a.ikm_stride;
    uint8_t ck[64], ikm[32], o1[64], o2[64];
    load_row(ck, a.ck, i, a.hl);
    for (int j = 0; j < 32; ++j) ikm[j] = ikm_p[j];
    kdf_hkdf(a.hash_id, a.hl, ck, a.hl, ikm, 32, o1, o2);
    store_row(a.ck, i, a.hl, o1);
    if (a.psk) {
        uint8_t h[64];
        load_row(h, a.h, i, a.hl);
        kdf_mix_hash(a.hash_id, a.hl, h, o2, a.hl);
        store_row(a.h, i, a.hl, h);
    } else {
        for (int j = 0; j < 32; ++j) a.k[(size_t)i * 32 + j] = o2[j];
    }
    if (a.zero_ikm)
        for (int j = 0; j < 32; ++j) ikm_p[j] = 0;
    for (int j = 0; j < 64; ++j) ck[j] = o1[j] = o2[j] = 0;
    for (int j = 0; j < 32; ++j) ikm[j] = 0;
}

__global__ __launch_bounds__(HS_BLOCK) void hs_null_check(const uint8_t *re, uint8_t *status, uint32_t n)
{
    const uint32_t i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= n || status[i]) return;
    uint8_t acc = 0;
    for (int j = 0; j < 32; ++j) acc |= re[(size_t)i * 32 + j];
    if (!acc) status[i] = HS_STATUS_NULL_KEY;
}

__global__ __launch_bounds__(HS_BLOCK) void hs_copy32(const uint8_t *src, uint64_t src_stride, uint8_t *dst, uint32_t n)
{
    const uint32_t i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= n) return;
    for (int j = 0; j < 32; ++j) dst[(size_t)i * 32 + j] = src[(uint64_t)i * src_stride + j];
}

struct BuildRecs {
    RecDesc *recs;
    const uint8_t *status;
    HsRows in_rows, out_rows;
    HsLens lens;
    uint64_t nonce, ctx_bytes;
    uint32_t hl, n;
};

__global__ __launch_bounds__(HS_BLOCK) void hs_build_recs(BuildRecs a)
{
    const uint32_t i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    RecDesc d;
    d.in_off = a.in_rows.at(i);
    d.out_off = a.out_rows.at(i);
    d.nonce = a.nonce;
    d.ctx_off = (uint64_t)i * a.ctx_bytes;
    d.ad_off = (uint64_t)i * a.hl;
    d.len = a.status[i] ? REFUSED_LEN : a.lens.payload(i);
    d.ad_len = a.hl;
    a.recs[i] = d;
}

struct SplitArgs {
    int hash_id;
    uint32_t hl, n;
    const uint8_t *ck, *h, *status;
    uint8_t *k1, *k2, *hh;
};

/* symmetricstate.c:530-533; a failed session's keys are zeros */
__global__ __launch_bounds__(HS_BLOCK) void hs_split(SplitArgs a)
{
    const uint32_t i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    uint8_t ck[64], o1[64], o2[64];
    load_row(ck, a.ck, i, a.hl);
    kdf_hkdf(a.hash_id, a.hl, ck, a.hl, nullptr, 0, o1, o2);
    const bool failed = a.status[i] != 0;
    for (int j = 0; j < 32; ++j) {
        a.k1[(size_t)i * 32 + j] = failed ? 0 : o1[j];
        a.k2[(size_t)i * 32 + j] = failed ? 0 : o2[j];
    }
    if (a.hh)
        for (uint32_t j = 0; j < a.hl; ++j) a.hh[(size_t)i * a.hl + j] = a.h[(size_t)i * a.hl + j];
    for (int j = 0; j < 64; ++j) ck[j] = o1[j] = o2[j] = 0;
}

/* noise_aead_dev_handshake_fallback: which sessions take part
   (hs_fallback_takes, handshake_plan.h) and the public values the new object
   keeps.  Session i's status in the new object is 0 or 5; a session that
   leaves the original with status 0 gets 5 there.  The former initiator's
   ephemeral public key and the local static public key are copied as they
   lie, one row when the key is shared. */
struct FallbackArgs {
    uint32_t n, flags, was_initiator;
    const uint8_t *select;
    uint8_t *hs_status, *fb_status;
    const uint8_t *e_src; /* the original's re (a former responder) or le_pub */
    uint8_t *e_dst;       /* the new object's re, or le_pub */
    uint64_t e_stride;    /* 0: one ephemeral for all, copied by lane 0 */
    const uint8_t *ls_src; /* NULL: the original never computed it */
    uint8_t *ls_dst;
    uint64_t ls_stride;
};

__global__ __launch_bounds__(HS_BLOCK) void hs_fallback_take(FallbackArgs a)
{
    const uint32_t i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const uint8_t st = a.hs_status[i];
    const bool takes = hs_fallback_takes(st, !a.select || a.select[i], a.flags, a.was_initiator);
    a.fb_status[i] = takes ? 0 : HS_STATUS_ABSENT;
    if (takes && !st) a.hs_status[i] = HS_STATUS_ABSENT;
    if (a.e_stride ? takes : i == 0)
        for (int j = 0; j < 32; ++j) a.e_dst[(size_t)i * a.e_stride + j] = a.e_src[(size_t)i * a.e_stride + j];
    if (a.ls_src && (a.ls_stride ? takes : i == 0))
        for (int j = 0; j < 32; ++j) a.ls_dst[(size_t)i * a.ls_stride + j] = a.ls_src[(size_t)i * a.ls_stride + j];
}

struct MergeArgs {
    uint32_t hl, n;
    const uint8_t *fb_status, *hs_status, *fb_k1, *fb_k2, *fb_h;
    uint8_t *k1, *k2, *h, *status;
};

/* noise_aead_dev_handshake_fallback_merge: the fallback's keys swapped into
   the original role's orientation, over the original's split */
__global__ __launch_bounds__(HS_BLOCK) void hs_fallback_merge(MergeArgs a)
{
    const uint32_t i = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const uint8_t st = a.fb_status[i];
    const HsMerge rule = hs_fallback_merge_rule(st);
    if (rule == HS_MERGE_KEEP) {
        a.status[i] = a.hs_status[i];
        return;
    }
    const bool take = rule == HS_MERGE_TAKE;
    for (int j = 0; j < 32; ++j) {
        a.k1[(size_t)i * 32 + j] = take ? a.fb_k2[(size_t)i * 32 + j] : 0;
        a.k2[(size_t)i * 32 + j] = take ? a.fb_k1[(size_t)i * 32 + j] : 0;
    }
    if (a.h)
        for (uint32_t j = 0; j < a.hl; ++j) a.h[(size_t)i * a.hl + j] = take ? a.fb_h[(size_t)i * a.hl + j] : 0;
    a.status[i] = st;
}

/* ---- sessions that change their object (header section 16).  What hs_move
   and hs_drop need of one object: its per-session rows.  A public-key row is
   per session at stride 32 (stride 0: one row for all, never moved or
   scrubbed); ls_priv / le_priv are read at their stride from wherever they
   lie, ls_own / le_own are the rows the object owns (NULL: none, the key is
   the caller's, shared or absent). */
struct LaneRows {
    uint32_t n;
    const uint32_t *lanes; /* NULL: entry j is lane j */
    uint8_t *ck, *h, *k, *ctx, *status, *re, *rs, *ls_pub, *le_pub;
    uint64_t ls_pub_stride, le_pub_stride;
    const uint8_t *ls_priv, *le_priv;
    uint64_t ls_stride, le_stride;
    uint8_t *ls_own, *le_own;
    __device__ __forceinline__ uint32_t lane(uint32_t j) const { return lanes ? lanes[j] : j; }
};

/* `bytes` (a multiple of 16) from one 16-byte aligned row of an arena to another, through registers */
__device__ __forceinline__ void move_row(uint8_t *dst, const uint8_t *src, uint32_t bytes)
{
    for (uint32_t j = 0; j < bytes; j += 16) *(uint4 *)(dst + j) = *(const uint4 *)(src + j);
}

__device__ __forceinline__ void zero_row(uint8_t *row, uint32_t bytes)
{
    for (uint32_t j = 0; j < bytes; j += 16) *(uint4 *)(row + j) = make_uint4(0, 0, 0, 0);
}

/* a private key from any address into an owned row: eight words in registers */
__device__ __forceinline__ void take_priv(uint8_t *own, const uint8_t *priv)
{
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        w[j] = (uint32_t)priv[4 * j] | (uint32_t)priv[4 * j + 1] << 8 | (uint32_t)priv[4 * j + 2] << 16 |
               (uint32_t)priv[4 * j + 3] << 24;
    *(uint4 *)own = make_uint4(w[0], w[1], w[2], w[3]);
    *(uint4 *)(own + 16) = make_uint4(w[4], w[5], w[6], w[7]);
}

/* every row of lane i that the object owns zeroed, the status 5 */
__device__ __forceinline__ void scrub_lane(const LaneRows &o, uint32_t i, uint32_t hl, uint32_t ctx_bytes)
{
    zero_row(o.ck + (size_t)i * hl, hl);
    zero_row(o.h + (size_t)i * hl, hl);
    zero_row(o.k + (size_t)i * 32, 32);
    zero_row(o.re + (size_t)i * 32, 32);
    zero_row(o.rs + (size_t)i * 32, 32);
    if (o.ls_pub_stride) zero_row(o.ls_pub + (size_t)i * 32, 32);
    if (o.le_pub_stride) zero_row(o.le_pub + (size_t)i * 32, 32);
    if (o.ls_own) zero_row(o.ls_own + (size_t)i * 32, 32);
    if (o.le_own) zero_row(o.le_own + (size_t)i * 32, 32);
    uint32_t *ctx = (uint32_t *)(o.ctx + (size_t)i * ctx_bytes);
    for (uint32_t j = 0; j < ctx_bytes / 4; ++j) ctx[j] = 0; /* 0 bytes under ChaChaPoly: its context is k */
    o.status[i] = HS_STATUS_ABSENT;
}

struct MoveArgs {
    LaneRows src, dst;
    uint32_t m, hl, ctx_bytes; /* ctx_bytes: of src's AES-GCM contexts, 0 under ChaChaPoly */
    uint8_t *result;
};

/* noise_aead_dev_handshake_move: entry j by hs_move_rule (handshake_plan.h) */
__global__ __launch_bounds__(HS_BLOCK) void hs_move(MoveArgs a)
{
    const uint32_t j = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (j >= a.m) return;
    const uint32_t s = a.src.lane(j), d = a.dst.lane(j);
    const bool in_range = s < a.src.n && d < a.dst.n;
    const uint8_t st = in_range ? a.src.status[s] : 0;
    const uint8_t r = hs_move_rule(s < a.src.n, d < a.dst.n, st, in_range ? a.dst.status[d] : 0);
    if (a.result) a.result[j] = r;
    if (r != NOISE_AEAD_MOVED) return;
    move_row(a.dst.ck + (size_t)d * a.hl, a.src.ck + (size_t)s * a.hl, a.hl);
    move_row(a.dst.h + (size_t)d * a.hl, a.src.h + (size_t)s * a.hl, a.hl);
    move_row(a.dst.k + (size_t)d * 32, a.src.k + (size_t)s * 32, 32);
    move_row(a.dst.re + (size_t)d * 32, a.src.re + (size_t)s * 32, 32);
    move_row(a.dst.rs + (size_t)d * 32, a.src.rs + (size_t)s * 32, 32);
    if (a.src.ls_pub_stride) move_row(a.dst.ls_pub + (size_t)d * 32, a.src.ls_pub + (size_t)s * 32, 32);
    if (a.src.le_pub_stride) move_row(a.dst.le_pub + (size_t)d * 32, a.src.le_pub + (size_t)s * 32, 32);
    if (a.dst.ls_own) take_priv(a.dst.ls_own + (size_t)d * 32, a.src.ls_priv + (uint64_t)s * a.src.ls_stride);
    if (a.dst.le_own) take_priv(a.dst.le_own + (size_t)d * 32, a.src.le_priv + (uint64_t)s * a.src.le_stride);
    scrub_lane(a.src, s, a.hl, a.ctx_bytes);
    a.dst.status[d] = st;
}

/* noise_aead_dev_handshake_drop */
__global__ __launch_bounds__(HS_BLOCK) void hs_drop(LaneRows o, uint32_t m, uint32_t hl, uint32_t ctx_bytes)
{
    const uint32_t j = blockIdx.x * HS_BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = o.lanes[j];
    if (i < o.n) scrub_lane(o, i, hl, ctx_bytes);
}

} // namespace

struct NoiseAeadDevHandshake {
    HsName name;
    bool fallback; /* the pattern is HS_XXFALLBACK, name.pattern the one it followed */
    int role, action, index;
    uint32_t n, hl;
    bool keyed, ctx_stale;
    uint64_t nonce;
    size_t ctx_bytes;
    /* the private keys (read by the DH steps): the caller's, or — per-session
       keys of an object from _new_like — the owned rows ls_own / le_own */
    const uint8_t *ls_priv, *le_priv;
    uint64_t ls_stride, le_stride;
    HsHold ls_hold, le_hold;
    bool made_like;
    uint8_t *ls_own, *le_own; /* parts of dev, or NULL */
    DevArena dev; /* the one device allocation; the pointers below are its parts */
    uint8_t *ck, *h, *k, *ctx, *arena, *status, *step, *ls_pub, *le_pub, *re, *rs;
    RecDesc *recs;
    uint64_t ls_pub_stride, le_pub_stride;
};

namespace {

typedef NoiseAeadDevHandshake Hs;

const HsPattern &pattern_of(const Hs *hs) { return hs->fallback ? HS_XXFALLBACK : HS_PATTERNS[hs->name.pattern]; }

HsMessage next_message(const Hs *hs) { return hs_message(pattern_of(hs), hs->role, hs->name.psk, hs->index, hs->keyed); }

/* One side of a message call: where the sessions' bytes are */
struct HsSpan {
    uint8_t *base;
    HsRows rows;
    HsSpan from(uint64_t off) const { return {base + off, rows}; } /* a token's bytes inside a message */
};

HsSpan strided(const uint8_t *base, uint64_t stride) { return {(uint8_t *)base, {nullptr, stride}}; }

HsLens fixed_len(uint32_t len) { return {nullptr, len, 0, 0}; }

int mix_hash(Hs *hs, HsSpan src, HsLens lens, uint32_t extra, HsSpan dst, const uint8_t *step, uint32_t *out_len,
             hipStream_t s)
{
    const MixHashArgs a = {hs->name.hash_id, hs->hl, hs->n, hs->h, src.base, src.rows, dst.base, dst.rows,
                           lens, extra, hs->status, step, out_len};
    return launch_items(hs_mix_hash, hs->n, HS_BLOCK, s, a);
}

/* MixHash of `len` bytes per session, with an optional copy */
int mix_hash(Hs *hs, HsSpan src, uint32_t len, HsSpan dst, hipStream_t s)
{
    return mix_hash(hs, src, fixed_len(len), 0, dst, nullptr, nullptr, s);
}

const HsSpan NO_COPY = {nullptr, {nullptr, 0}};

int mix_key(Hs *hs, const uint8_t *ikm, uint64_t ikm_stride, bool zero_ikm, bool psk, hipStream_t s)
{
    const MixKeyArgs a = {hs->name.hash_id, hs->hl, hs->n, hs->ck, hs->k, hs->h, (uint8_t *)ikm, ikm_stride,
                          zero_ikm, psk};
    const int rc = launch_items(hs_mix_key, hs->n, HS_BLOCK, s, a);
    if (!psk) {
        hs->keyed = true;
        hs->nonce = 0;
        hs->ctx_stale = true;
    }
    return rc;
}

/* encrypt_and_hash / decrypt_and_hash of each session's lens.payload(i) bytes
   once a key is set: seal or open under AD = h, then h = HASH(h || CT || tag)
   — after an open only where the tag verified */
int aead_step(Hs *hs, bool open, HsSpan in, HsSpan out, HsLens lens, uint32_t *out_len, hipStream_t s)
{
    const int cipher = hs->name.cipher_id;
    int rc = NOISE_ERROR_NONE;
    if (cipher == NOISE_CIPHER_AESGCM && hs->ctx_stale)
        rc = noise_aead_dev_prepare(cipher, hs->k, hs->n, hs->ctx, s);
    hs->ctx_stale = false;
    if (rc) return rc;
    /* an empty payload may come without a pointer; the ragged job wants one */
    if (!in.base) in = strided(hs->arena, 0);
    if (!out.base) out = strided(hs->arena, 0);
    const BuildRecs b = {hs->recs, hs->status, in.rows, out.rows, lens, hs->nonce, hs->ctx_bytes, hs->hl, hs->n};
    rc = launch_items(hs_build_recs, hs->n, HS_BLOCK, s, b);
    if (rc) return rc;
    NoiseAeadRagged job = {};
    job.ctx_base = cipher == NOISE_CIPHER_AESGCM ? hs->ctx : hs->k;
    job.recs = (const NoiseAeadRecord *)hs->recs;
    job.in = in.base;
    job.out = out.base;
    job.ad = hs->h;
    job.status = hs->step;
    job.n_records = hs->n;
    rc = open ? noise_aead_dev_open_ragged(cipher, &job, s) : noise_aead_dev_seal_ragged(cipher, &job, s);
    if (rc) return rc;
    ++hs->nonce;
    return open ? mix_hash(hs, in, lens, HS_MAC_LEN, NO_COPY, hs->step, out_len, s)
                : mix_hash(hs, out, lens, HS_MAC_LEN, NO_COPY, nullptr, out_len, s);
}

int dh_step(Hs *hs, const HsStep &st, hipStream_t s)
{
    const uint8_t *priv = st.priv_static ? hs->ls_priv : hs->le_priv;
    const uint64_t priv_stride = st.priv_static ? hs->ls_stride : hs->le_stride;
    const int rc = noise_aead_dev_dh_calculate(NOISE_DH_CURVE25519, priv, priv_stride, st.pub_static ? hs->rs : hs->re,
                                               HS_DH_LEN, hs->n, hs->arena, s);
    return rc ? rc : mix_key(hs, hs->arena, HS_DH_LEN, true, false, s);
}

/* The tokens and the payload of the next message; write: payload -> msg.
   lens.per (a ragged call): the length rule first, and out_len with the
   payload step, the last launch, where the statuses of this call are final. */
int run_message(Hs *hs, const HsMessage &m, bool write, HsSpan msg, HsSpan payload, HsLens lens, uint32_t *out_len,
                hipStream_t s)
{
    uint64_t off = 0;
    int rc = NOISE_ERROR_NONE;
    if (lens.per) rc = launch_items(hs_check_len, hs->n, HS_BLOCK, s, lens, hs->status, hs->n);
    const HsSpan ls_pub = strided(hs->ls_pub, hs->ls_pub_stride), le_pub = strided(hs->le_pub, hs->le_pub_stride);
    const HsSpan re = strided(hs->re, HS_DH_LEN), rs = strided(hs->rs, HS_DH_LEN);
    for (int t = 0; t < m.n_steps && !rc; ++t) {
        const HsStep &st = m.steps[t];
        const HsSpan at = msg.from(off);
        switch (st.kind) {
        case HS_STEP_E:
            if (write) {
                rc = mix_hash(hs, le_pub, HS_DH_LEN, at, s);
                if (!rc && st.mix_key) rc = mix_key(hs, hs->le_pub, hs->le_pub_stride, false, false, s);
            } else {
                rc = mix_hash(hs, at, HS_DH_LEN, re, s);
                if (!rc) rc = launch_items(hs_null_check, hs->n, HS_BLOCK, s, hs->re, hs->status, hs->n);
                if (!rc && st.mix_key) rc = mix_key(hs, hs->re, HS_DH_LEN, false, false, s);
            }
            off += HS_DH_LEN;
            break;
        case HS_STEP_S:
            if (write)
                rc = st.keyed ? aead_step(hs, false, ls_pub, at, fixed_len(HS_DH_LEN), nullptr, s)
                              : mix_hash(hs, ls_pub, HS_DH_LEN, at, s);
            else
                rc = st.keyed ? aead_step(hs, true, at, rs, fixed_len(HS_DH_LEN), nullptr, s)
                              : mix_hash(hs, at, HS_DH_LEN, rs, s);
            off += HS_DH_LEN + (st.keyed ? HS_MAC_LEN : 0);
            break;
        case HS_STEP_DH:
            rc = dh_step(hs, st, s);
            break;
        case HS_STEP_PAYLOAD:
            if (write)
                rc = st.keyed ? aead_step(hs, false, payload, at, lens, out_len, s)
                              : mix_hash(hs, payload, lens, 0, at, nullptr, out_len, s);
            else
                rc = st.keyed ? aead_step(hs, true, at, payload, lens, out_len, s)
                              : mix_hash(hs, at, lens, 0, payload, nullptr, out_len, s);
            break;
        }
    }
    return rc;
}

void advance(Hs *hs, const HsMessage &m)
{
    hs->keyed = m.keyed_after;
    hs->action = m.next_action;
    ++hs->index;
}

/* h and ck of the name, MixHash(prologue), the PSK step
   (symmetricstate.c:97-108, handshakestate.c:822-842) */
int start_symmetric(Hs *hs, const char *name, const uint8_t *d_prologue, uint64_t prologue_stride, uint32_t prologue_len,
                    const uint8_t *d_psk, uint64_t psk_stride, hipStream_t s)
{
    InitArgs ia = {};
    ia.hash_id = hs->name.hash_id;
    ia.hl = hs->hl;
    ia.n = hs->n;
    ia.name_len = (uint32_t)strlen(name);
    ia.h = hs->h;
    ia.ck = hs->ck;
    memcpy(ia.name, name, ia.name_len);
    int rc = launch_items(hs_init, hs->n, HS_BLOCK, s, ia);
    if (!rc) rc = mix_hash(hs, strided(prologue_len ? d_prologue : hs->arena, prologue_stride), prologue_len, NO_COPY, s);
    if (!rc && hs->name.psk) rc = mix_key(hs, d_psk, psk_stride, false, true, s);
    return rc;
}

/* the device arrays of an object of n > 0 sessions; own_ls, own_le: rows of
   its own for the private keys as well (_new_like) */
bool carve(Hs *hs, bool own_ls = false, bool own_le = false)
{
    const size_t n = hs->n;
    DevArena &d = hs->dev;
    d.align = HS_ALIGN;
    const size_t o_ck = d.carve(n * hs->hl), o_h = d.carve(n * hs->hl), o_k = d.carve(n * 32);
    const size_t o_ctx = d.carve(hs->name.cipher_id == NOISE_CIPHER_AESGCM ? n * hs->ctx_bytes : 0);
    const size_t o_arena = d.carve(n * 32), o_status = d.carve(n), o_step = d.carve(n);
    const size_t o_ls = d.carve(n * 32), o_le = d.carve(n * 32), o_re = d.carve(n * 32);
    const size_t o_rs = d.carve(n * 32), o_recs = d.carve(n * sizeof(RecDesc));
    const size_t o_ls_own = d.carve(own_ls ? n * 32 : 0), o_le_own = d.carve(own_le ? n * 32 : 0);
    if (!d.alloc()) return false;
    hs->ls_own = own_ls ? d.at(o_ls_own) : nullptr;
    hs->le_own = own_le ? d.at(o_le_own) : nullptr;
    hs->ck = d.at(o_ck); hs->h = d.at(o_h); hs->k = d.at(o_k); hs->ctx = d.at(o_ctx); hs->arena = d.at(o_arena);
    hs->status = d.at(o_status); hs->step = d.at(o_step); hs->ls_pub = d.at(o_ls); hs->le_pub = d.at(o_le);
    hs->re = d.at(o_re); hs->rs = d.at(o_rs); hs->recs = d.at<RecDesc>(o_recs);
    return true;
}

/* everything _fallback launches, after the allocation: who takes part and
   what fb keeps, a former responder's fresh ephemeral, the start-up with the
   new name, then the pre-message e (handshakestate.c:848-857, :864-873) */
int start_fallback(Hs *fb, Hs *hs, const NoiseAeadHandshakeFallbackConfig *cfg, const char *name, hipStream_t s)
{
    const bool init = hs_is_initiator(fb->role); /* the former responder */
    int rc = fb->dev.zero(s);
    if (rc) return rc;
    FallbackArgs a = {};
    a.n = hs->n;
    a.flags = cfg->flags;
    a.was_initiator = !init;
    a.select = cfg->d_select;
    a.hs_status = hs->status;
    a.fb_status = fb->status;
    a.e_src = init ? hs->re : hs->le_pub;
    a.e_dst = init ? fb->re : fb->le_pub;
    a.e_stride = init ? HS_DH_LEN : hs->le_pub_stride;
    /* a static key the original pattern had no use for has no public key yet */
    const bool have_ls_pub = hs_needs(pattern_of(hs), hs->role).local_static;
    a.ls_src = have_ls_pub ? hs->ls_pub : nullptr;
    a.ls_dst = fb->ls_pub;
    a.ls_stride = hs->ls_pub_stride;
    rc = launch_items(hs_fallback_take, hs->n, HS_BLOCK, s, a);
    if (!rc && !have_ls_pub)
        rc = noise_aead_dev_dh_public(NOISE_DH_CURVE25519, fb->ls_priv, fb->ls_stride, fb->ls_stride ? fb->n : 1,
                                      fb->ls_pub, s);
    if (!rc && init)
        rc = noise_aead_dev_dh_public(NOISE_DH_CURVE25519, fb->le_priv, fb->le_stride, fb->le_stride ? fb->n : 1,
                                      fb->le_pub, s);
    if (!rc)
        rc = start_symmetric(fb, name, cfg->d_prologue, cfg->prologue_stride, cfg->prologue_len, cfg->d_psk,
                             cfg->psk_stride, s);
    const uint8_t *e = init ? fb->re : fb->le_pub;
    const uint64_t e_stride = init ? HS_DH_LEN : fb->le_pub_stride;
    if (!rc) rc = mix_hash(fb, strided(e, e_stride), HS_DH_LEN, NO_COPY, s);
    if (!rc && fb->name.psk) rc = mix_key(fb, e, e_stride, false, false, s);
    return rc;
}

/* everything _new launches, after the allocation */
int start(Hs *hs, const NoiseAeadHandshakeConfig *cfg, hipStream_t s)
{
    const HsPattern &p = pattern_of(hs);
    const HsNeeds need = hs_needs(p, hs->role);
    int rc = hs->dev.zero(s);
    /* the local public keys: one ladder launch each, one lane for a shared key */
    if (!rc && need.local_static)
        rc = noise_aead_dev_dh_public(NOISE_DH_CURVE25519, hs->ls_priv, hs->ls_stride, hs->ls_stride ? hs->n : 1,
                                      hs->ls_pub, s);
    if (!rc && need.local_ephemeral)
        rc = noise_aead_dev_dh_public(NOISE_DH_CURVE25519, hs->le_priv, hs->le_stride, hs->le_stride ? hs->n : 1,
                                      hs->le_pub, s);
    if (!rc && need.remote_static)
        rc = launch_items(hs_copy32, hs->n, HS_BLOCK, s, cfg->d_remote_static_pub, cfg->remote_static_stride, hs->rs,
                          hs->n);
    if (!rc)
        rc = start_symmetric(hs, cfg->protocol_name, cfg->d_prologue, cfg->prologue_stride, cfg->prologue_len, cfg->d_psk,
                             cfg->psk_stride, s);
    /* :844-877 */
    const bool init = hs_is_initiator(hs->role);
    const HsSpan ls_pub = strided(hs->ls_pub, hs->ls_pub_stride), rs = strided(hs->rs, HS_DH_LEN);
    if (!rc && p.pre_i_s) rc = mix_hash(hs, init ? ls_pub : rs, HS_DH_LEN, NO_COPY, s);
    if (!rc && p.pre_r_s) rc = mix_hash(hs, init ? rs : ls_pub, HS_DH_LEN, NO_COPY, s);
    return rc;
}

} // namespace

extern "C" {

int noise_aead_dev_handshake_new(NoiseAeadDevHandshake **out, const NoiseAeadHandshakeConfig *cfg, void *stream)
{
    if (!out) return NOISE_ERROR_INVALID_PARAM;
    *out = nullptr;
    HsName name;
    int rc = hs_check_config(cfg, &name);
    if (rc) return rc;
    if (strlen(cfg->protocol_name) > HS_NAME_MAX) return NOISE_ERROR_UNKNOWN_NAME; /* no name in scope is */
    Hs *hs = new (std::nothrow) Hs();
    if (!hs) return NOISE_ERROR_NO_MEMORY;
    hs->name = name;
    hs->role = cfg->role;
    hs->action = hs_first_action(cfg->role);
    hs->n = cfg->n;
    hs->hl = hash_len(name.hash_id);
    hs->ctx_bytes = noise_aead_dev_ctx_bytes(name.cipher_id);
    hs->ls_priv = cfg->d_local_static_priv;
    hs->ls_stride = cfg->local_static_stride;
    hs->le_priv = cfg->d_local_ephemeral_priv;
    hs->le_stride = cfg->local_ephemeral_stride;
    hs->ls_pub_stride = hs->ls_stride ? HS_DH_LEN : 0;
    hs->le_pub_stride = hs->le_stride ? HS_DH_LEN : 0;
    hs->ls_hold = hs_hold_of(hs->ls_priv, hs->ls_stride);
    hs->le_hold = hs_hold_of(hs->le_priv, hs->le_stride);
    if (hs->n) {
        if (!carve(hs)) {
            delete hs;
            return NOISE_ERROR_NO_MEMORY;
        }
        rc = start(hs, cfg, (hipStream_t)stream);
        if (rc) {
            noise_aead_dev_handshake_free(hs);
            return rc;
        }
    }
    *out = hs;
    return NOISE_ERROR_NONE;
}

int noise_aead_dev_handshake_free(NoiseAeadDevHandshake *hs)
{
    if (!hs) return NOISE_ERROR_INVALID_PARAM;
    const int rc = hs->dev.release();
    memset((void *)hs, 0, sizeof(*hs));
    delete hs;
    return rc;
}

int noise_aead_dev_handshake_get_action(const NoiseAeadDevHandshake *hs) { return hs ? hs->action : NOISE_ACTION_NONE; }

size_t noise_aead_dev_handshake_overhead(const NoiseAeadDevHandshake *hs)
{
    if (!hs || (hs->action != NOISE_ACTION_WRITE_MESSAGE && hs->action != NOISE_ACTION_READ_MESSAGE)) return 0;
    return next_message(hs).overhead;
}

int noise_aead_dev_handshake_write_message(NoiseAeadDevHandshake *hs, const uint8_t *d_payload,
                                           uint64_t payload_stride, uint32_t payload_len, uint8_t *d_msg,
                                           uint64_t msg_stride, void *stream)
{
    if (!hs) return NOISE_ERROR_INVALID_PARAM;
    if (hs->action != NOISE_ACTION_WRITE_MESSAGE) return NOISE_ERROR_INVALID_STATE;
    const HsMessage m = next_message(hs);
    int rc = hs_check_write(hs->action, hs->n, m.overhead, d_payload, payload_stride, payload_len, d_msg, msg_stride);
    if (rc) return rc;
    if (hs->n)
        rc = run_message(hs, m, true, strided(d_msg, msg_stride), strided(d_payload, payload_stride),
                         fixed_len(payload_len), nullptr, (hipStream_t)stream);
    advance(hs, m);
    return rc;
}

int noise_aead_dev_handshake_write_message_ragged(NoiseAeadDevHandshake *hs, const uint8_t *d_payload,
                                                  const uint64_t *d_payload_off, const uint32_t *d_payload_len,
                                                  uint8_t *d_msg, const uint64_t *d_msg_off, uint32_t *d_msg_len,
                                                  void *stream)
{
    int rc = hs_check_write_ragged(hs, hs ? hs->action : NOISE_ACTION_NONE, hs ? hs->n : 0, d_payload, d_payload_off,
                                   d_payload_len, d_msg, d_msg_off, d_msg_len);
    if (rc) return rc;
    const HsMessage m = next_message(hs);
    if (hs->n) {
        /* without the payload triple every payload is empty: the fixed length 0 */
        const HsLens lens = {d_payload_len, 0, m.overhead, 1};
        rc = run_message(hs, m, true, HsSpan{d_msg, {d_msg_off, 0}}, HsSpan{(uint8_t *)d_payload, {d_payload_off, 0}}, lens,
                         d_msg_len, (hipStream_t)stream);
    }
    advance(hs, m);
    return rc;
}

int noise_aead_dev_handshake_read_message_ragged(NoiseAeadDevHandshake *hs, const uint8_t *d_msg,
                                                 const uint64_t *d_msg_off, const uint32_t *d_msg_len,
                                                 uint8_t *d_payload, const uint64_t *d_payload_off,
                                                 uint32_t *d_payload_len, void *stream)
{
    int rc = hs_check_read_ragged(hs, hs ? hs->action : NOISE_ACTION_NONE, hs ? hs->n : 0, d_msg, d_msg_off, d_msg_len,
                                  d_payload, d_payload_off, d_payload_len);
    if (rc) return rc;
    const HsMessage m = next_message(hs);
    if (hs->n) {
        const HsLens lens = {d_msg_len, 0, m.overhead, 0};
        rc = run_message(hs, m, false, HsSpan{(uint8_t *)d_msg, {d_msg_off, 0}}, HsSpan{d_payload, {d_payload_off, 0}}, lens,
                         d_payload_len, (hipStream_t)stream);
    }
    advance(hs, m);
    return rc;
}

int noise_aead_dev_handshake_read_message(NoiseAeadDevHandshake *hs, const uint8_t *d_msg, uint64_t msg_stride,
                                          uint32_t msg_len, uint8_t *d_payload, uint64_t payload_stride,
                                          void *stream)
{
    if (!hs) return NOISE_ERROR_INVALID_PARAM;
    if (hs->action != NOISE_ACTION_READ_MESSAGE) return NOISE_ERROR_INVALID_STATE;
    const HsMessage m = next_message(hs);
    int rc = hs_check_read(hs->action, hs->n, m.overhead, d_msg, msg_stride, msg_len, d_payload, payload_stride);
    if (rc) return rc;
    if (hs->n)
        rc = run_message(hs, m, false, strided(d_msg, msg_stride), strided(d_payload, payload_stride),
                         fixed_len(msg_len - m.overhead), nullptr, (hipStream_t)stream);
    advance(hs, m);
    return rc;
}

int noise_aead_dev_handshake_split(NoiseAeadDevHandshake *hs, uint8_t *d_k1, uint8_t *d_k2,
                                   uint8_t *d_handshake_hash, void *stream)
{
    if (!hs) return NOISE_ERROR_INVALID_PARAM;
    int rc = hs_check_split(hs->action, hs->n, hs->hl, d_k1, d_k2, d_handshake_hash);
    if (rc) return rc;
    if (hs->n) {
        const SplitArgs a = {hs->name.hash_id, hs->hl, hs->n, hs->ck, hs->h, hs->status, d_k1, d_k2, d_handshake_hash};
        rc = launch_items(hs_split, hs->n, HS_BLOCK, (hipStream_t)stream, a);
    }
    hs->action = NOISE_ACTION_COMPLETE;
    return rc;
}

int noise_aead_dev_handshake_fallback(NoiseAeadDevHandshake *hs, const NoiseAeadHandshakeFallbackConfig *cfg,
                                      NoiseAeadDevHandshake **out, void *stream)
{
    if (out) *out = nullptr;
    HsFallbackFrom from = {};
    if (hs) from = {&pattern_of(hs), hs->name.psk, hs->role, hs->action, hs->index, hs->ls_hold != HS_HOLD_NONE, hs->made_like};
    int rc = hs_check_fallback(from, cfg, out);
    if (rc) return rc;
    char name[HS_NAME_MAX];
    if (!hs_fallback_name(hs->name, name, sizeof(name))) return NOISE_ERROR_INVALID_LENGTH;
    Hs *fb = new (std::nothrow) Hs();
    if (!fb) return NOISE_ERROR_NO_MEMORY;
    const bool init = !hs_is_initiator(hs->role); /* the roles swap (handshakestate.c:1035-1046) */
    fb->name = hs->name;
    fb->fallback = true;
    fb->role = init ? NOISE_ROLE_INITIATOR : NOISE_ROLE_RESPONDER;
    fb->action = hs_first_action(fb->role);
    fb->n = hs->n;
    fb->hl = hs->hl;
    fb->ctx_bytes = hs->ctx_bytes;
    fb->ls_priv = hs->ls_priv;
    fb->ls_stride = hs->ls_stride;
    fb->ls_pub_stride = hs->ls_pub_stride;
    fb->le_priv = init ? cfg->d_local_ephemeral_priv : hs->le_priv;
    fb->le_stride = init ? cfg->local_ephemeral_stride : hs->le_stride;
    fb->le_pub_stride = fb->le_stride ? HS_DH_LEN : 0;
    fb->ls_hold = hs_hold_of(fb->ls_priv, fb->ls_stride);
    fb->le_hold = hs_hold_of(fb->le_priv, fb->le_stride);
    if (fb->n) {
        if (!carve(fb)) {
            delete fb;
            return NOISE_ERROR_NO_MEMORY;
        }
        rc = start_fallback(fb, hs, cfg, name, (hipStream_t)stream);
        if (rc) {
            noise_aead_dev_handshake_free(fb);
            return rc;
        }
    } else {
        fb->keyed = hs_keyed_before(HS_XXFALLBACK, fb->name.psk, 0);
    }
    *out = fb;
    return NOISE_ERROR_NONE;
}

int noise_aead_dev_handshake_fallback_merge(const NoiseAeadDevHandshake *fb, const uint8_t *d_hs_status,
                                            uint8_t *d_k1, uint8_t *d_k2, const uint8_t *d_fb_k1,
                                            const uint8_t *d_fb_k2, uint8_t *d_h, const uint8_t *d_fb_h,
                                            uint8_t *d_status, void *stream)
{
    const int rc = hs_check_fallback_merge(fb, fb ? fb->action : NOISE_ACTION_NONE, fb ? fb->n : 0, fb ? fb->hl : 0,
                                           fb ? fb->status : nullptr, d_hs_status, d_k1, d_k2, d_fb_k1, d_fb_k2, d_h,
                                           d_fb_h, d_status);
    if (rc || !fb->n) return rc;
    const MergeArgs a = {fb->hl, fb->n, fb->status, d_hs_status, d_fb_k1, d_fb_k2, d_fb_h, d_k1, d_k2, d_h, d_status};
    return launch_items(hs_fallback_merge, fb->n, HS_BLOCK, (hipStream_t)stream, a);
}

int noise_aead_dev_handshake_new_like(NoiseAeadDevHandshake **out, const NoiseAeadDevHandshake *like,
                                      uint32_t capacity, void *stream)
{
    if (out) *out = nullptr;
    int rc = hs_check_new_like(out, like, like ? like->action : NOISE_ACTION_NONE);
    if (rc) return rc;
    Hs *hs = new (std::nothrow) Hs();
    if (!hs) return NOISE_ERROR_NO_MEMORY;
    hs->name = like->name;
    hs->fallback = like->fallback;
    hs->role = like->role;
    hs->action = like->action;
    hs->index = like->index;
    hs->n = capacity;
    hs->hl = like->hl;
    hs->keyed = like->keyed;
    hs->ctx_stale = like->keyed;
    hs->nonce = like->nonce;
    hs->ctx_bytes = like->ctx_bytes;
    hs->made_like = true;
    hs->ls_hold = like->ls_hold;
    hs->le_hold = like->le_hold;
    hs->ls_pub_stride = like->ls_pub_stride;
    hs->le_pub_stride = like->le_pub_stride;
    const bool own_ls = hs->ls_hold == HS_HOLD_EACH, own_le = hs->le_hold == HS_HOLD_EACH;
    if (hs->n && !carve(hs, own_ls, own_le)) {
        delete hs;
        return NOISE_ERROR_NO_MEMORY;
    }
    /* per session: the owned rows (NULL with no lanes); once for all: like's pointer */
    hs->ls_priv = own_ls ? hs->ls_own : like->ls_priv;
    hs->ls_stride = own_ls ? HS_DH_LEN : like->ls_stride;
    hs->le_priv = own_le ? hs->le_own : like->le_priv;
    hs->le_stride = own_le ? HS_DH_LEN : like->le_stride;
    if (hs->n) {
        hipStream_t s = (hipStream_t)stream;
        rc = hs->dev.zero(s);
        if (!rc) rc = hip_rc(hipMemsetAsync(hs->status, HS_STATUS_ABSENT, hs->n, s));
        /* the one public-key row of a shared key (an object of no lanes has none to copy) */
        if (!rc && like->n && hs->ls_hold == HS_HOLD_SHARED)
            rc = launch_items(hs_copy32, 1, HS_BLOCK, s, (const uint8_t *)like->ls_pub, (uint64_t)0, hs->ls_pub, 1u);
        if (!rc && like->n && hs->le_hold == HS_HOLD_SHARED)
            rc = launch_items(hs_copy32, 1, HS_BLOCK, s, (const uint8_t *)like->le_pub, (uint64_t)0, hs->le_pub, 1u);
        if (rc) {
            noise_aead_dev_handshake_free(hs);
            return rc;
        }
    }
    *out = hs;
    return NOISE_ERROR_NONE;
}

namespace {

LaneRows lane_rows(const Hs *hs, const uint32_t *d_lanes)
{
    return {hs->n, d_lanes, hs->ck, hs->h, hs->k, hs->ctx, hs->status, hs->re, hs->rs, hs->ls_pub, hs->le_pub,
            hs->ls_pub_stride, hs->le_pub_stride, hs->ls_priv, hs->le_priv, hs->ls_stride, hs->le_stride,
            hs->ls_own, hs->le_own};
}

HsMoveSide move_side(const Hs *hs, const uint32_t *d_lanes)
{
    if (!hs) return {};
    return {hs,
            {hs->name, hs->fallback, hs->role, hs->action, hs->index, hs->keyed, hs->nonce},
            {{hs->ls_hold, hs->ls_priv, hs->made_like}, {hs->le_hold, hs->le_priv, hs->made_like}},
            hs->n,
            d_lanes};
}

uint32_t aes_ctx_bytes(const Hs *hs) { return hs->name.cipher_id == NOISE_CIPHER_AESGCM ? (uint32_t)hs->ctx_bytes : 0; }

} // namespace

int noise_aead_dev_handshake_move(NoiseAeadDevHandshake *dst, const uint32_t *d_dst_lanes, NoiseAeadDevHandshake *src,
                                  const uint32_t *d_src_lanes, uint32_t m, uint8_t *d_result, void *stream)
{
    const int rc = hs_check_move(move_side(dst, d_dst_lanes), move_side(src, d_src_lanes), m, d_result);
    if (rc || !m) return rc;
    if (dst->keyed) dst->ctx_stale = true; /* the contexts are not moved: prepared from k, as after a MixKey */
    const MoveArgs a = {lane_rows(src, d_src_lanes), lane_rows(dst, d_dst_lanes), m, src->hl, aes_ctx_bytes(src), d_result};
    return launch_items(hs_move, m, HS_BLOCK, (hipStream_t)stream, a);
}

int noise_aead_dev_handshake_drop(NoiseAeadDevHandshake *hs, const uint32_t *d_lanes, uint32_t m, void *stream)
{
    const int rc = hs_check_drop(hs, hs ? hs->n : 0, d_lanes, m);
    if (rc || !m) return rc;
    return launch_items(hs_drop, m, HS_BLOCK, (hipStream_t)stream, lane_rows(hs, d_lanes), m, hs->hl, aes_ctx_bytes(hs));
}

const uint8_t *noise_aead_dev_handshake_status(const NoiseAeadDevHandshake *hs) { return hs ? hs->status : nullptr; }

const uint8_t *noise_aead_dev_handshake_remote_static(const NoiseAeadDevHandshake *hs) { return hs ? hs->rs : nullptr; }

} // extern "C"
