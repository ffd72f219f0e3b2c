/*
 * transport_plan.h — the host-only half of the device-resident transport
 * sessions (noise_aead_dev_transport_*, include/noise_aead_hip.h section 9):
 * the frame walk of one session, the cap rule across sessions, the slot of a
 * call's entry (section 10, the session table), the anti-replay window of the
 * datagram calls (section 11), the counter blocks and the direction rule of
 * rekey (section 12), the classification, the sort key, the run walk and the
 * judging rule of the packet calls (section 13), the packet echo's rule for one
 * packet (section 14), and the argument checks.  One
 * source for both compilers, as fe25519.h is: hipcc's
 * device pass builds the kernels of transport.hip from tr_walk and tr_cap,
 * plain g++ builds asan/transport_check.cpp, asan/transport_table_check.cpp,
 * asan/transport_datagram_check.cpp, asan/transport_rekey_check.cpp,
 * asan/transport_packet_check.cpp and asan/transport_packet_echo_check.cpp from
 * them, so the CPU check under ASan/UBSan runs the walk, the window rule, the
 * direction rule and the run walk the GPU runs.
 *
 * The wire format is that of csrc/wire.c (echo-common.c:643-688): a 2-byte
 * big-endian length L, then L bytes of CT || tag; in a datagram frame the L
 * bytes start with the frame's 8-byte little-endian counter.
 */
#pragma once
#include "noise_aead_hip.h"
#include <stdint.h>

#if defined(__HIPCC__)
#define TR_FN __host__ __device__ __forceinline__
#define TR_MEMBER __host__ __device__ __forceinline__
#else
#define TR_FN static inline __attribute__((always_inline))
#define TR_MEMBER inline
#endif

namespace na {

constexpr uint64_t TR_NONCE_LIMIT = ~0ull;     /* cipherstate.c: n == 2^64 - 1 is exhausted */
constexpr uint32_t TR_MAC_LEN = 16;
constexpr uint32_t TR_MAX_FRAMES = 1u << 31;   /* the most records one call may describe */
constexpr uint64_t TR_NO_BUDGET = ~0ull;
constexpr uint32_t TR_COUNTER_LEN = 8;                             /* a datagram frame's counter */
constexpr uint32_t TR_DATAGRAM_MIN = TR_COUNTER_LEN + TR_MAC_LEN;  /* its smallest L */
constexpr uint32_t TR_REPLAY_BITS = 1024;                          /* the anti-replay window */
constexpr uint32_t TR_REPLAY_WORDS = TR_REPLAY_BITS / 64;

struct TrWalk {
    uint64_t frames;    /* frames taken */
    uint64_t consumed;  /* bytes they span, headers included */
    int32_t stop;       /* why the walk ended: NOISE_ERROR_NONE / _INVALID_LENGTH / _INVALID_NONCE */
};

/* a frame the walk took: emit(k, body, L) with body the offset of its L bytes in the stream */
struct TrNoEmit {
    TR_MEMBER void operator()(uint64_t, uint64_t, uint32_t) const {}
};

/* The walk of one session's stream, in the order of wire.c scan_frames: the
   frames from the start of p[0..len), frame k under nonce + k.  It ends with
   NOISE_ERROR_NONE at a partial (or absent) frame, with _INVALID_LENGTH at a
   complete frame with L < min_len (16: a tag; 24 for a datagram frame, which
   carries its counter), with _INVALID_NONCE where nonce + k is
   2^64 - 1; the stopping frame is not taken.  A frame that would be taken as
   number `budget` is left for the next call instead: the walk ends there with
   NOISE_ERROR_NONE, having taken `budget` frames — so a stop that comes
   right after the budget's last frame is still reported.  For an echo, nonce
   is the larger of the two directions' (the first to run out).  Reads only
   p[0..len). */
template <class Emit>
TR_FN TrWalk tr_walk(const uint8_t *p, uint64_t len, uint64_t nonce, uint64_t budget, Emit emit,
                     uint32_t min_len = TR_MAC_LEN)
{
    TrWalk w = {0, 0, NOISE_ERROR_NONE};
    uint64_t off = 0;
    while (len - off >= 2) {
        const uint32_t L = ((uint32_t)p[off] << 8) | p[off + 1];
        if (len - off - 2 < L) break;
        /* both the tag of seal and the MAC of open need L >= 16 (cipherstate.c:305-318 / :379-390) */
        if (L < min_len) {
            w.stop = NOISE_ERROR_INVALID_LENGTH;
            break;
        }
        if (nonce + w.frames == TR_NONCE_LIMIT) { /* nonce + frames never wraps: it stops here first */
            w.stop = NOISE_ERROR_INVALID_NONCE;
            break;
        }
        if (w.frames == budget) break;
        emit(w.frames, off + 2, L);
        off += 2 + (uint64_t)L;
        ++w.frames;
    }
    w.consumed = off;
    return w;
}

TR_FN TrWalk tr_walk(const uint8_t *p, uint64_t len, uint64_t nonce, uint64_t budget)
{
    return tr_walk(p, len, nonce, budget, TrNoEmit());
}

/* The cap across sessions.  The walked frames of a call are numbered in
   session order; a session whose uncapped walk takes `count` frames starts at
   number `base` (the exclusive sum of the counts before it, in 64 bits).  What
   the session may take in a call over max_frames records: everything when its
   frames all lie below max_frames (its walk then reports its own stop), else
   the frames below max_frames (none from base == max_frames on) and the call
   reports NOISE_ERROR_NONE for it: it did not reach its stop.  A session after
   the cut takes nothing.  Returns the budget of the session's walk; *cut says
   the session reports NOISE_ERROR_NONE whatever its walk met. */
TR_FN uint64_t tr_cap(uint64_t base, uint64_t count, uint64_t max_frames, bool *cut)
{
    *cut = count > max_frames || base > max_frames - count; /* base + count > max_frames, without a wrap */
    if (!*cut) return count;
    return base < max_frames ? max_frames - base : 0;
}

/* The slot of entry j of a call (section 10): slots[j], or j itself for the
   calls that take no list (slots == NULL).  Returns whether it names one of
   the object's n slots; an entry that does not is skipped by every kernel,
   which resolves its slot through this one function.  Reads only slots[j]. */
TR_FN bool tr_slot(const uint32_t *slots, uint32_t j, uint32_t n, uint32_t *i)
{
    *i = slots ? slots[j] : j;
    return *i < n;
}

/* ------------------------------------------------- the anti-replay window
   Section 11.  The state of one slot: top is the highest accepted counter
   + 1 (0: nothing accepted yet); bit c % 1024 of seen says counter c was
   accepted, for the 1024 counters top - 1024 .. top - 1.  The layout is what
   noise_aead_dev_transport_replay hands out. */
struct TrReplay {
    uint64_t top;
    uint64_t seen[TR_REPLAY_WORDS];
};

/* Whether counter c is fresh against the window: not 2^64 - 1 (the CipherState
   never uses that nonce), not older than the window, not seen.  Reads only. */
TR_FN bool tr_replay_check(const TrReplay *w, uint64_t c)
{
    if (c == TR_NONCE_LIMIT) return false;
    if (c >= w->top) return true;
    if (w->top - c > TR_REPLAY_BITS) return false;
    return !((w->seen[(c / 64) % TR_REPLAY_WORDS] >> (c % 64)) & 1);
}

/* Counter c, which tr_replay_check found fresh, is accepted.  At or above top
   the window moves: the bits of the counters top .. c - 1, which nobody has
   seen, are cleared (all of them when the jump is a window or more), and top
   becomes c + 1.  Then c's bit is set. */
TR_FN void tr_replay_accept(TrReplay *w, uint64_t c)
{
    if (c >= w->top) {
        if (c - w->top >= TR_REPLAY_BITS) {
            for (uint32_t q = 0; q < TR_REPLAY_WORDS; ++q) w->seen[q] = 0;
        } else {
            for (uint64_t x = w->top; x < c;) { /* a word's share of top .. c - 1 at a time; c <= 2^64 - 2 */
                const uint64_t bit = x % 64, span = c - x < 64 - bit ? c - x : 64 - bit;
                const uint64_t mask = (span == 64 ? ~0ull : (1ull << span) - 1) << bit;
                w->seen[(x / 64) % TR_REPLAY_WORDS] &= ~mask;
                x += span;
            }
        }
        w->top = c + 1;
    }
    w->seen[(c / 64) % TR_REPLAY_WORDS] |= 1ull << (c % 64);
}

/* ------------------------------------------------------------------ rekey
   Section 12.  REKEY(k) is the first 32 bytes of ENCRYPT(k, 2^64 - 1, "", 32
   zero bytes): key stream alone, no tag. */

/* ChaChaPoly: bytes 0..31 of the block under counter 1 (counter 0 is the
   Poly1305 key) and the 64-bit IV LE64(2^64 - 1) */
constexpr uint32_t TR_REKEY_CHACHA_COUNTER = 1;
constexpr uint32_t TR_REKEY_CHACHA_IV_LO = 0xffffffffu, TR_REKEY_CHACHA_IV_HI = 0xffffffffu;

/* AES-GCM: the CTR blocks 2 and 3 under J0 = 0^32 || BE64(2^64 - 1) || BE32(1);
   word w of block b (0, 1) as aes256_block takes it, big-endian */
TR_FN uint32_t tr_rekey_aes_word(uint32_t b, uint32_t w)
{
    return w == 0 ? 0u : (w < 3 ? 0xffffffffu : 2u + b);
}

/* The directions a call rekeys for entry j: `directions` (bit 0 send, bit 1
   receive) masked by the entry's byte of d_which, all of it without one. */
TR_FN uint32_t tr_rekey_directions(uint32_t directions, const uint8_t *which, uint32_t j)
{
    return directions & (which ? which[j] : 3u);
}

/* ------------------------------------------------------ packet transport
   Section 13.  A call's packets come in list order with their slots repeated
   and interleaved.  Each packet gets a sort key, a stable sort of (key,
   position in the list) brings every slot's packets together with their list
   order kept, and one lane walks a slot's run. */

constexpr uint8_t TR_STATUS_AEAD_REFUSED = 2;  /* the ragged kernels' answer to refused_rec(): nothing was done */
constexpr uint8_t TR_STATUS_LENGTH = 4;
constexpr uint8_t TR_STATUS_REPLAY = 5;
constexpr uint8_t TR_STATUS_NO_SESSION = 6;
constexpr uint32_t TR_PACKET_MAX_LEN = 65535;
constexpr uint32_t TR_MAX_PACKETS = 1u << 31;  /* the most packets an object may reserve for */

/* What keeps a packet out of the call, in the order of the header: 6 (no such
   slot, or unkeyed), 4 (its length), else 0.  Reads only keyed[slot], and that
   only for a slot of the table. */
TR_FN uint8_t tr_packet_class(uint32_t slot, uint32_t len, uint32_t n, const uint8_t *keyed)
{
    if (slot >= n || !keyed[slot]) return TR_STATUS_NO_SESSION;
    if (len < TR_DATAGRAM_MIN || len > TR_PACKET_MAX_LEN) return TR_STATUS_LENGTH;
    return 0;
}

/* The sort key: the slot, or n, the sentinel of a packet that takes no part;
   the sentinels sort behind every slot's run. */
TR_FN uint32_t tr_packet_key(uint8_t cls, uint32_t slot, uint32_t n)
{
    return cls ? n : slot;
}

/* the bits of a key: the fewest that hold n, and at least one */
TR_FN uint32_t tr_packet_key_bits(uint32_t n)
{
    uint32_t bits = 1;
    while (bits < 32 && (n >> bits)) ++bits;
    return bits;
}

/* whether sorted position q is the first of a slot's run */
TR_FN bool tr_run_head(const uint32_t *keys, uint32_t q, uint32_t n)
{
    return keys[q] != n && (q == 0 || keys[q - 1] != keys[q]);
}

/* The run that starts at sorted position q, in list order (the sort is
   stable): visit(p) for each of its packets, p the packet's place in the
   list.  Reads keys[q .. end of the run], one key past it when there is one,
   and as much of order. */
template <class Visit>
TR_FN void tr_run_walk(const uint32_t *keys, const uint32_t *order, uint32_t count, uint32_t q, Visit visit)
{
    const uint32_t slot = keys[q];
    for (; q < count && keys[q] == slot; ++q) visit(order[q]);
}

/* The open's rule for one packet, frame or counter c against the window as
   the ones before it left it; s is the AEAD's status of it (2: the window as
   it stood before the call refused it, nothing was opened).  Refused before or
   by now -> 5; the tag failed -> 1; else c is accepted -> 0.  Refusal is
   monotone over a call: what the window refused before the call
   it refuses at every later point of it, so judging the pre-checked packets
   in order gives what one-by-one processing gives. */
TR_FN uint8_t tr_replay_judge(TrReplay *w, uint64_t c, uint8_t s)
{
    if (s == TR_STATUS_AEAD_REFUSED || !tr_replay_check(w, c)) return TR_STATUS_REPLAY;
    if (s == 0) tr_replay_accept(w, c);
    return s;
}

/* The seal's counter for the next sealed packet of a slot: *c = send, and send
   moves on; false, and nothing moves, where that counter would be 2^64 - 1. */
TR_FN bool tr_seal_take(uint64_t *send, uint64_t *c)
{
    if (*send == TR_NONCE_LIMIT) return false;
    *c = (*send)++;
    return true;
}

/* The echo's rule for one packet (section 14): the open's, then the seal's
   for what the open accepted.  w is the slot's window and *send the lane's
   copy of its send counter, both as the packets before this one left them; c
   is the counter the packet came with and s the AEAD's status of its open.
   What tr_replay_judge refuses keeps that status and takes no counter.  An
   accepted packet has moved the window; it then takes the next send counter
   into *taken -> 0, or finds it run out -> 5, with the window still moved. */
TR_FN uint8_t tr_echo_judge(TrReplay *w, uint64_t *send, uint64_t c, uint8_t s, uint64_t *taken)
{
    const uint8_t opened = tr_replay_judge(w, c, s);
    if (opened) return opened;
    return tr_seal_take(send, taken) ? 0 : TR_STATUS_REPLAY;
}

/* --------------------------------------------------------- argument checks
   Pointers are compared as numbers and never dereferenced. */

typedef unsigned __int128 tr_u128;

/* [a, a + a_bytes) meets [b, b + b_bytes) */
inline bool tr_ranges_meet(const void *a, tr_u128 a_bytes, const void *b, tr_u128 b_bytes)
{
    if (!a_bytes || !b_bytes) return false;
    const tr_u128 x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

/* noise_aead_dev_transport_new, in the order of the header */
inline int tr_check_new(const void *out, int cipher_id, int role, uint32_t n, const void *d_k1, const void *d_k2,
                        uint32_t max_frames)
{
    if (cipher_id != NOISE_CIPHER_CHACHAPOLY && cipher_id != NOISE_CIPHER_AESGCM) return NOISE_ERROR_UNKNOWN_ID;
    if (role != NOISE_ROLE_INITIATOR && role != NOISE_ROLE_RESPONDER) return NOISE_ERROR_INVALID_PARAM;
    if (!out || !d_k1 || !d_k2) return NOISE_ERROR_INVALID_PARAM;
    if (n && (max_frames == 0 || max_frames > TR_MAX_FRAMES)) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* ---- the session table (section 10), each in the order of the header.  A
   check that returns NOISE_ERROR_NONE with m == 0 means: nothing to launch. */

/* noise_aead_dev_transport_new_unkeyed: _new's checks without the key pointers */
inline int tr_check_new_unkeyed(const void *out, int cipher_id, int role, uint32_t n, uint32_t max_frames)
{
    return tr_check_new(out, cipher_id, role, n, out, out, max_frames);
}

/* noise_aead_dev_transport_set_keys on an object of n slots (d_status may be NULL) */
inline int tr_check_set_keys(const void *tr, uint32_t n, const void *d_slots, uint32_t m, const void *d_k1,
                             const void *d_k2)
{
    if (!tr) return NOISE_ERROR_INVALID_PARAM;
    if (!m) return NOISE_ERROR_NONE;
    if (m > n) return NOISE_ERROR_INVALID_PARAM;
    if (!d_slots || !d_k1 || !d_k2) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* noise_aead_dev_transport_clear_keys */
inline int tr_check_clear_keys(const void *tr, uint32_t n, const void *d_slots, uint32_t m)
{
    if (!tr) return NOISE_ERROR_INVALID_PARAM;
    if (!m) return NOISE_ERROR_NONE;
    if (m > n || !d_slots) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* noise_aead_dev_transport_rekey (section 12) on an object of n slots; d_slots
   and d_which may be NULL, so no pointer but tr is looked at */
inline int tr_check_rekey(const void *tr, uint32_t n, uint32_t m, uint32_t directions)
{
    if (!tr) return NOISE_ERROR_INVALID_PARAM;
    if (!m) return NOISE_ERROR_NONE;
    if (m > n) return NOISE_ERROR_INVALID_PARAM;
    if (directions == 0 || directions > (NOISE_AEAD_REKEY_SEND | NOISE_AEAD_REKEY_RECEIVE)) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

/* ---- the frame calls of sections 9 to 11: one set of rules, in the order of
   the header.  The form says what a call takes: TR_FORM_ALL (section 9) has no
   list and is about all n slots, and looks at its pointers even when n == 0;
   TR_FORM_OF (section 10) needs its list; TR_FORM_DATAGRAM (section 11) may
   have one.  For the last two m == 0 means: nothing to launch.
   result_bytes: of one entry's result; d_frame_status, the datagram open's,
   is an argument when frame_status is set: [d_frame_status, + the call's cap). */
enum TrForm { TR_FORM_ALL, TR_FORM_OF, TR_FORM_DATAGRAM };

inline int tr_check_frames(TrForm form, const void *tr, uint32_t n, uint32_t object_max_frames, const void *d_slots,
                           uint32_t m, uint32_t max_frames, const void *d_wire, const void *d_off, const void *d_len,
                           const void *d_result, uint32_t result_bytes, bool frame_status, const void *d_frame_status)
{
    if (!tr) return NOISE_ERROR_INVALID_PARAM;
    if (!m && form != TR_FORM_ALL) return NOISE_ERROR_NONE;
    if (m > n) return NOISE_ERROR_INVALID_PARAM;
    if ((form == TR_FORM_OF && !d_slots) || !d_wire || !d_off || !d_len || !d_result || (frame_status && !d_frame_status))
        return NOISE_ERROR_INVALID_PARAM;
    if (max_frames > object_max_frames) return NOISE_ERROR_INVALID_PARAM;
    const tr_u128 rb = (tr_u128)result_bytes * m, ob = (tr_u128)8 * m, lb = (tr_u128)4 * m, sb = d_slots ? lb : 0;
    if (tr_ranges_meet(d_result, rb, d_off, ob) || tr_ranges_meet(d_result, rb, d_len, lb) ||
        tr_ranges_meet(d_result, rb, d_slots, sb))
        return NOISE_ERROR_INVALID_PARAM;
    if (frame_status) {
        const tr_u128 fb = max_frames ? max_frames : object_max_frames;
        if (tr_ranges_meet(d_frame_status, fb, d_off, ob) || tr_ranges_meet(d_frame_status, fb, d_len, lb) ||
            tr_ranges_meet(d_frame_status, fb, d_slots, sb) || tr_ranges_meet(d_frame_status, fb, d_result, rb))
            return NOISE_ERROR_INVALID_PARAM;
    }
    return NOISE_ERROR_NONE;
}

/* noise_aead_dev_transport_{seal,open,echo}_frames of an object of n sessions */
inline int tr_check_call(const void *tr, uint32_t n, const void *d_wire, const void *d_off, const void *d_len,
                         const void *d_result)
{
    return tr_check_frames(TR_FORM_ALL, tr, n, 0, nullptr, n, 0, d_wire, d_off, d_len, d_result,
                           sizeof(NoiseAeadTransportResult), false, nullptr);
}

/* noise_aead_dev_transport_{seal,open,echo}_frames_of on an object of n slots
   made for object_max_frames records */
inline int tr_check_call_of(const void *tr, uint32_t n, uint32_t object_max_frames, const void *d_slots, uint32_t m,
                            uint32_t max_frames, const void *d_wire, const void *d_off, const void *d_len,
                            const void *d_result)
{
    return tr_check_frames(TR_FORM_OF, tr, n, object_max_frames, d_slots, m, max_frames, d_wire, d_off, d_len, d_result,
                           sizeof(NoiseAeadTransportResult), false, nullptr);
}

/* noise_aead_dev_transport_{seal,open}_datagrams: result_bytes is 16 for the
   seal, 24 for the open, which also takes d_frame_status */
inline int tr_check_datagrams(const void *tr, uint32_t n, uint32_t object_max_frames, const void *d_slots, uint32_t m,
                              uint32_t max_frames, const void *d_wire, const void *d_off, const void *d_len,
                              const void *d_result, uint32_t result_bytes, bool open, const void *d_frame_status)
{
    return tr_check_frames(TR_FORM_DATAGRAM, tr, n, object_max_frames, d_slots, m, max_frames, d_wire, d_off, d_len,
                           d_result, result_bytes, open, d_frame_status);
}

/* ---- the packet calls of section 13, in the order of the header.
   reserved_packets: what the object has reserved for, 0 when it has not. */

/* noise_aead_dev_transport_reserve_packets; the allocation comes after it */
inline int tr_check_reserve_packets(const void *tr, uint32_t max_packets, uint32_t reserved_packets)
{
    if (!tr) return NOISE_ERROR_INVALID_PARAM;
    if (max_packets == 0 || max_packets > TR_MAX_PACKETS) return NOISE_ERROR_INVALID_PARAM;
    if (reserved_packets) return NOISE_ERROR_INVALID_STATE;
    return NOISE_ERROR_NONE;
}

/* noise_aead_dev_transport_{seal,open}_packets and _echo_packets (section 14);
   NOISE_ERROR_NONE with count == 0 means: nothing to launch */
inline int tr_check_packets(const void *tr, uint32_t reserved_packets, const void *d_packets, uint32_t count,
                            const void *d_wire, const void *d_status)
{
    if (!tr) return NOISE_ERROR_INVALID_PARAM;
    if (!count) return NOISE_ERROR_NONE;
    if (!reserved_packets) return NOISE_ERROR_INVALID_STATE;
    if (count > reserved_packets) return NOISE_ERROR_INVALID_PARAM;
    if (!d_packets || !d_wire || !d_status) return NOISE_ERROR_INVALID_PARAM;
    if (tr_ranges_meet(d_status, count, d_packets, (tr_u128)sizeof(NoiseAeadPacket) * count)) return NOISE_ERROR_INVALID_PARAM;
    return NOISE_ERROR_NONE;
}

} // namespace na
