/*
 * transport.hip — device-resident transport sessions:
 * noise_aead_dev_transport_* (include/noise_aead_hip.h sections 9 to 14).
 *
 * The object holds, for n sessions, a send and a receive key context and a
 * send and a receive nonce on the device, and what a call needs: descriptors
 * and statuses for max_frames records, per-session counts and bases, scan
 * scratch — all of it one DevArena (launch.h), zeroed before use and zeroed
 * again before it is freed.  The per-session and per-entry kernels go out
 * through launch_items (launch.h); a descriptor nothing may be done for is
 * refused_rec() (aead_kernels.h).
 *
 * A call is handed every session's bytes in the echo wire format and does per
 * session what noise_wire_seal / _open / _echo do (wire.c), with nothing
 * coming back to the host:
 *   tr_count   one lane per session walks its headers (transport_plan.h
 *              tr_walk, no budget) and leaves its frame count;
 *   the scan   rocprim's exclusive scan of the 64-bit counts: the number of
 *              each session's first frame in the batch;
 *   tr_build   one lane per session applies the cap (tr_cap), walks again and
 *              writes its frames' descriptors (in place, nonce + k, the
 *              session's context, no AD) from its base on; lanes past the
 *              last frame pad the array up to max_frames with descriptors the
 *              ragged kernels refuse (status 2, nothing written).  A seal
 *              commits here: the send nonce advances, the result is written;
 *   the AEAD   noise_aead_dev_{seal,open}_ragged over max_frames records,
 *              any alignment (frames sit at 2-byte offsets), automatic lanes;
 *              the total is known only on the device;
 *   tr_commit  open and echo: one lane per session finds its first frame
 *              whose status is not 0, advances the nonce(s) by that prefix
 *              and writes the result; for an echo it also writes the seal
 *              descriptors: the prefix under the send state, the rest refused.
 *
 * The session table (section 10): every slot has a state byte (keyed or not),
 * and a call may name the m slots it is about in a device list.  Entry j of
 * such a call is slot tr_slot(slots, j) (transport_plan.h): the caller's
 * arrays and the per-call scratch are indexed by j, nonces, contexts and
 * state by the slot; an entry out of range or unkeyed counts no frames and
 * gets its fixed result from tr_build.  The calls of section 9 are the list
 * NULL (entry j is slot j), m == n and the object's own cap.  The AEAD
 * launches cover the call's cap, not the object's.
 *   tr_set_keys  ChaChaPoly, one lane per entry: both contexts (the context is
 *                the key), both nonces, the state; an entry whose status byte
 *                is not 0 is cleared instead.  AES-GCM builds its contexts
 *                with gcm_prepare_slots (aesgcm.hip), then tr_clear_wide marks
 *                the entries and zeroes the failed ones;
 *   tr_clear_lane / tr_clear_wide  _clear_keys: zero both contexts with 16-byte
 *                stores, both nonces and the state; a lane per entry for the
 *                32-byte ChaChaPoly contexts, a workgroup per (entry,
 *                direction) for the 41 344-byte AES-GCM ones.
 *
 * Datagram transport (section 11): every frame carries its counter, every
 * frame is judged alone, and each slot has an anti-replay window (TrReplay,
 * transport_plan.h) that tr_mark zeroes with the nonces.  A call is the same
 * run (run(), below) under the other framing: tr_count<TR_DATAGRAM>, the scan,
 *   tr_build<TR_DATAGRAM>  the one build kernel with the datagram emitter.
 *                Seal: writes frame k's counter send + k and its descriptor
 *                (in place behind the counter).  Open: reads each frame's
 *                counter, asks tr_replay_check of the window as it stands, and
 *                writes the descriptor under that counter or refused_rec(): a
 *                replay costs no AEAD work;
 *   the AEAD     as above, the open verify-first;
 *   tr_commit_datagrams  open: one lane per entry walks its frames in order
 *                with the window evolving: refused before (status 2) or by
 *                now -> 5, tag failed -> 1, else tr_replay_accept -> 0.
 *
 * Rekey (section 12): a key, or a slot's key context, becomes its successor
 * REKEY(k) on the device in stream order; nonces, windows and state bytes are
 * not touched.
 *   tr_rekey_keys / tr_rekey_slots  ChaChaPoly: one ChaCha20 block in registers
 *                (tr_rekey_chacha), a lane per key, or per (entry, direction)
 *                in place on the object's contexts: the context is the key;
 *   AES-GCM      gcm_rekey_keys / gcm_rekey_slots (aesgcm.hip), next to the
 *                tables: the two blocks under the context's own round keys,
 *                then the context rebuilt by gcm_prepare_one.
 *
 * Packet transport (section 13): the datagram calls over a device list of
 * {off, len, slot} in arrival order, slots repeated and interleaved; one
 * status byte per packet.  What a call needs (TrPackets) is an allocation of
 * its own that _reserve_packets makes; descriptor p belongs to packet p, and
 * the AEAD launch covers exactly the call's count:
 *   tr_packet_keys    one lane per packet: its class (6, 4 or 0) to d_status,
 *                its sort key (the slot, or n for a packet that takes no
 *                part), order[p] = p, and its descriptor: refused_rec(), or,
 *                for a live packet of an open, what tr_build<TR_DATAGRAM>
 *                writes for a frame after asking the window as it stands;
 *   the sort     rocprim's radix sort of (key, order) over the bits of n; it
 *                is stable, so a slot's packets keep their list order;
 *   tr_packet_seal    seal: the lane at the head of a slot's run (tr_run_walk)
 *                hands out send, send + 1, .. in list order (tr_seal_take),
 *                writes each counter and descriptor, gives 5 from exhaustion
 *                on and advances send;
 *   the AEAD     as above, over count records;
 *   tr_packet_commit  open: the lane at the head of a run judges its packets
 *                in list order with the window evolving (tr_replay_judge, the
 *                rule of tr_commit_datagrams).
 *
 * Packet echo (section 14): an open of the list and the seal of what it
 * accepted, in place, in one call: tr_packet_keys as for the open, the sort,
 * the AEAD's open over count records, then
 *   tr_packet_echo    in tr_packet_commit's place: the lane at the head of a
 *                run reads the slot's send once and walks the run once
 *                (tr_echo_judge): each packet against the evolving window, and
 *                an accepted one takes the next send counter, gets it written
 *                in front and its descriptor rewritten in place as the seal's;
 *                every other packet of the run gets refused_rec();
 *   the AEAD     the seal over the same count descriptors, no statuses.
 */
#include "launch.h"

#include "aead_device.h"
#include "transport_plan.h"

#include <new>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

using namespace na;

namespace {

#define TR_DEV __device__ __forceinline__

constexpr uint32_t TR_BLOCK = 64;
constexpr uint32_t TR_WIDE_BLOCK = 256;
constexpr size_t TR_ALIGN = 256; /* of the parts of the object's device allocation */

enum TrMode : uint32_t { TR_SEAL = 0, TR_OPEN = 1, TR_ECHO = 2 };
/* how a session's frames are laid out, named by the smallest L of a frame;
   the datagram calls are TR_SEAL or TR_OPEN only */
enum TrFraming : uint32_t { TR_STREAM = TR_MAC_LEN, TR_DATAGRAM = TR_DATAGRAM_MIN };

struct TrArgs {
    uint8_t *wire;               /* written only by the datagram seal: its counters */
    const uint64_t *off;
    const uint32_t *len;
    NoiseAeadTransportResult *result; /* not the datagram open's */
    uint64_t *send, *recv;       /* the nonces */
    uint64_t *count, *base;      /* per session: frames of the uncapped walk, their exclusive sum */
    uint32_t *frames, *consumed; /* per session, after the cap */
    int32_t *stop;
    RecDesc *recs, *seal_recs;   /* max_frames each; seal_recs: the echo's second job */
    const uint8_t *status;
    uint64_t ctx_bytes, max_frames; /* max_frames: this call's cap */
    uint32_t n, mode;
    const uint32_t *slots;       /* the call's list (null: entry j is slot j) of m entries */
    const uint8_t *keyed;        /* per slot: 1 keyed, 0 not */
    uint32_t m;
    /* the datagram calls'; null for the stream calls */
    TrReplay *replay;            /* per slot */
    NoiseAeadDatagramResult *datagram_result; /* the open's */
    uint8_t *frame_status;       /* the open's, one byte per walked frame of the call */
};

/* entry j's slot; false (nothing of a slot may be touched) when it is out of range or unkeyed */
TR_DEV bool tr_live(const TrArgs &a, uint32_t j, uint32_t *i)
{
    return tr_slot(a.slots, j, a.n, i) && a.keyed[*i];
}

/* the nonce the walk of a stream starts under */
TR_DEV uint64_t tr_start_nonce(const TrArgs &a, uint32_t i)
{
    if (a.mode == TR_SEAL) return a.send[i];
    if (a.mode == TR_OPEN) return a.recv[i];
    return a.send[i] > a.recv[i] ? a.send[i] : a.recv[i];
}

template <TrFraming F>
__global__ __launch_bounds__(TR_BLOCK) void tr_count(TrArgs a)
{
    const uint32_t j = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (j >= a.m) return;
    uint32_t i;
    uint64_t count = 0;
    if (tr_live(a, j, &i)) {
        const uint64_t nonce = F == TR_DATAGRAM && a.mode == TR_OPEN ? 0 : tr_start_nonce(a, i); /* a datagram open walks under none */
        count = tr_walk(a.wire + a.off[j], a.len[j], nonce, TR_NO_BUDGET, TrNoEmit(), F).frames;
    }
    a.count[j] = count;
}

/* lane t's share of the padding: the descriptors from the call's last frame
   up to its cap are ones the ragged kernels refuse */
TR_DEV void tr_pad(const TrArgs &a, RecDesc *recs, uint64_t t)
{
    const uint64_t all = a.base[a.m - 1] + a.count[a.m - 1];
    const uint64_t total = all < a.max_frames ? all : a.max_frames;
    if (t >= total && t < a.max_frames) recs[t] = refused_rec();
}

/* a frame's descriptor: len bytes in place at `at` of the wire, no AD */
TR_DEV RecDesc tr_rec(uint64_t at, uint64_t nonce, uint64_t ctx_off, uint32_t len)
{
    RecDesc d;
    d.in_off = d.out_off = at;
    d.nonce = nonce;
    d.ctx_off = ctx_off;
    d.ad_off = 0;
    d.len = len;
    d.ad_len = 0;
    return d;
}

/* a stream frame k: under nonce + k */
struct TrEmit {
    RecDesc *recs;
    uint64_t wire_off, nonce, ctx_off;
    TR_DEV void operator()(uint64_t k, uint64_t body, uint32_t L) const
    {
        recs[k] = tr_rec(wire_off + body, nonce + k, ctx_off, L - TR_MAC_LEN);
    }
};

static_assert(TR_STATUS_AEAD_REFUSED == STATUS_BAD_LENGTH, "what the ragged kernels answer to refused_rec()");

/* nothing of a stream is aligned */
TR_DEV uint64_t tr_load_counter(const uint8_t *p)
{
    uint64_t c = 0;
    for (int b = 0; b < 8; ++b) c |= (uint64_t)p[b] << (8 * b);
    return c;
}

/* a datagram frame k: behind the counter, under that counter; the seal writes
   send + k there first, the open refuses what the window refuses */
struct TrDatagramEmit {
    RecDesc *recs;
    uint8_t *stream;             /* the entry's */
    uint64_t wire_off, send, ctx_off;
    const TrReplay *window;      /* null: a seal */
    TR_DEV void operator()(uint64_t k, uint64_t body, uint32_t L) const
    {
        uint64_t c = send + k;
        if (window)
            c = tr_load_counter(stream + body);
        else
            for (int b = 0; b < 8; ++b) stream[body + b] = (uint8_t)(c >> (8 * b));
        const bool fresh = !window || tr_replay_check(window, c);
        recs[k] = fresh ? tr_rec(wire_off + body + TR_COUNTER_LEN, c, ctx_off, L - TR_DATAGRAM_MIN) : refused_rec();
    }
};

template <TrFraming F>
__global__ __launch_bounds__(TR_BLOCK) void tr_build(TrArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    tr_pad(a, a.recs, t);
    if (t >= a.m) return;
    const uint32_t j = (uint32_t)t;
    const bool seal = a.mode == TR_SEAL;
    uint32_t i;
    if (!tr_live(a, j, &i)) { /* before anything else, cut or not (wire.c:199); the commit leaves the entry alone */
        const int32_t error = i < a.n ? NOISE_ERROR_INVALID_STATE : NOISE_ERROR_INVALID_PARAM;
        if (F == TR_DATAGRAM && !seal) {
            const NoiseAeadDatagramResult r = {0, 0, error, 0, 0};
            a.datagram_result[j] = r;
        } else {
            const NoiseAeadTransportResult r = {0, 0, error, 0};
            a.result[j] = r;
        }
        return;
    }
    bool cut;
    const uint64_t base = a.base[j], budget = tr_cap(base, a.count[j], a.max_frames, &cut);
    const bool walk = budget || !cut;
    /* the session's context: send contexts first, then the receive ones */
    const uint64_t ctx_off = (seal ? (uint64_t)i : (uint64_t)a.n + i) * a.ctx_bytes;
    uint8_t *stream = a.wire + a.off[j];
    TrWalk w = {0, 0, NOISE_ERROR_NONE};
    if constexpr (F == TR_STREAM) {
        const TrEmit emit = {a.recs + base, a.off[j], seal ? a.send[i] : a.recv[i], ctx_off};
        if (walk) w = tr_walk(stream, a.len[j], tr_start_nonce(a, i), budget, emit, F);
    } else {
        const uint64_t send = seal ? a.send[i] : 0; /* the open neither walks under a nonce nor reads one */
        const TrDatagramEmit emit = {a.recs + base, stream, a.off[j], send, ctx_off, seal ? nullptr : a.replay + i};
        if (walk) w = tr_walk(stream, a.len[j], send, budget, emit, F);
    }
    if (cut) w.stop = NOISE_ERROR_NONE;
    if (seal) {
        a.send[i] += w.frames;
        const NoiseAeadTransportResult r = {(uint32_t)w.frames, (uint32_t)w.consumed, w.stop, 0};
        a.result[j] = r;
        return;
    }
    a.frames[j] = (uint32_t)w.frames;
    a.consumed[j] = (uint32_t)w.consumed;
    a.stop[j] = w.stop;
}

__global__ __launch_bounds__(TR_BLOCK) void tr_commit(TrArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    const bool echo = a.mode == TR_ECHO;
    if (echo) tr_pad(a, a.seal_recs, t);
    if (t >= a.m) return;
    const uint32_t j = (uint32_t)t;
    uint32_t i;
    if (!tr_live(a, j, &i)) return; /* tr_build wrote its result; it has no frames */
    const uint32_t frames = a.frames[j];
    const uint64_t base = a.base[j]; /* base + frames <= max_frames (tr_cap); not read when frames == 0 */
    uint32_t prefix = 0;
    while (prefix < frames && a.status[base + prefix] == 0) ++prefix;
    NoiseAeadTransportResult r = {prefix, a.consumed[j], a.stop[j], 0};
    if (prefix < frames) { /* the first tag that failed wins over a later stop (wire.c wire_run) */
        r.consumed = (uint32_t)(a.recs[base + prefix].in_off - 2 - a.off[j]);
        r.error = NOISE_ERROR_MAC_FAILURE;
    }
    if (echo) {
        const uint64_t send = a.send[i];
        for (uint32_t k = 0; k < frames; ++k) {
            RecDesc d = refused_rec();
            if (k < prefix) {
                d = a.recs[base + k];
                d.nonce = send + k;
                d.ctx_off = (uint64_t)i * a.ctx_bytes;
            }
            a.seal_recs[base + k] = d;
        }
        a.send[i] = send + prefix;
    }
    a.recv[i] += prefix; /* it stays at the failed frame's nonce (cipherstate.c:400-405) */
    a.result[j] = r;
}

/* frame k of the entry, in stream order, against the window as the frames before it left it */
struct TrDatagramJudge {
    const uint8_t *stream, *status; /* the entry's; the AEAD's statuses from the entry's first frame on */
    uint8_t *frame_status;
    TrReplay *window;
    uint32_t *accepted;
    TR_DEV void operator()(uint64_t k, uint64_t body, uint32_t) const
    {
        const uint64_t c = tr_load_counter(stream + body);
        const uint8_t out = tr_replay_judge(window, c, status[k]);
        if (out == 0) ++*accepted;
        frame_status[k] = out;
    }
};

__global__ __launch_bounds__(TR_BLOCK) void tr_commit_datagrams(TrArgs a)
{
    const uint32_t j = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (j >= a.m) return;
    uint32_t i;
    if (!tr_live(a, j, &i)) return; /* tr_build wrote its result; it has no frames */
    const uint32_t frames = a.frames[j];
    const uint64_t base = a.base[j]; /* base + frames <= max_frames (tr_cap) */
    uint32_t accepted = 0;
    if (frames) { /* the headers and counters are as tr_build read them: the same frames again */
        const TrDatagramJudge judge = {a.wire + a.off[j], a.status + base, a.frame_status + base, a.replay + i, &accepted};
        tr_walk(a.wire + a.off[j], a.len[j], 0, frames, judge, TR_DATAGRAM_MIN);
    }
    const NoiseAeadDatagramResult r = {frames, a.consumed[j], a.stop[j], accepted, base};
    a.datagram_result[j] = r;
}

/* ---- packet transport (section 13) */

struct TrPacketArgs {
    const NoiseAeadPacket *packets; /* the caller's list of `count` */
    uint8_t *wire;
    uint8_t *status;             /* the caller's, one byte per packet */
    uint32_t *keys, *order;      /* tr_packet_keys: what the sort reads; after it: what the sort left */
    RecDesc *recs;               /* descriptor p is packet p's */
    const uint8_t *aead_status;  /* the open's, per packet */
    uint64_t *send;
    TrReplay *replay;
    const uint8_t *keyed;
    uint64_t ctx_bytes;
    uint32_t n, count, mode;     /* TR_SEAL, TR_OPEN or TR_ECHO */
};

__global__ __launch_bounds__(TR_BLOCK) void tr_packet_keys(TrPacketArgs a)
{
    const uint32_t p = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (p >= a.count) return;
    const NoiseAeadPacket pk = a.packets[p];
    const uint8_t cls = tr_packet_class(pk.slot, pk.len, a.n, a.keyed);
    a.keys[p] = tr_packet_key(cls, pk.slot, a.n);
    a.order[p] = p;
    a.status[p] = cls;
    RecDesc d = refused_rec(); /* a seal's live packets get theirs from tr_packet_seal */
    if (a.mode != TR_SEAL && !cls) {
        const uint64_t c = tr_load_counter(a.wire + pk.off);
        if (tr_replay_check(a.replay + pk.slot, c)) /* else: a replay costs no AEAD work */
            d = tr_rec(pk.off + TR_COUNTER_LEN, c, ((uint64_t)a.n + pk.slot) * a.ctx_bytes, pk.len - TR_DATAGRAM_MIN);
    }
    a.recs[p] = d;
}

/* a packet of a slot's run under the seal: the next counter in front and its descriptor, or 5 */
struct TrPacketSeal {
    const TrPacketArgs &a;
    uint64_t *send;              /* the lane's copy of the slot's */
    uint64_t ctx_off;
    TR_DEV void operator()(uint32_t p) const
    {
        uint64_t c;
        if (!tr_seal_take(send, &c)) {
            a.status[p] = TR_STATUS_REPLAY;
            return;
        }
        const NoiseAeadPacket pk = a.packets[p];
        for (int b = 0; b < 8; ++b) a.wire[pk.off + b] = (uint8_t)(c >> (8 * b));
        a.recs[p] = tr_rec(pk.off + TR_COUNTER_LEN, c, ctx_off, pk.len - TR_DATAGRAM_MIN);
    }
};

__global__ __launch_bounds__(TR_BLOCK) void tr_packet_seal(TrPacketArgs a)
{
    const uint32_t q = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (q >= a.count || !tr_run_head(a.keys, q, a.n)) return;
    const uint32_t i = a.keys[q];
    uint64_t send = a.send[i];
    tr_run_walk(a.keys, a.order, a.count, q, TrPacketSeal{a, &send, (uint64_t)i * a.ctx_bytes});
    a.send[i] = send;
}

/* a packet of a slot's run under the open, against the window as the packets before it left it */
struct TrPacketJudge {
    const TrPacketArgs &a;
    TrReplay *window;
    TR_DEV void operator()(uint32_t p) const
    {
        /* the counter is the descriptor's nonce; a refused descriptor has none, and needs none */
        a.status[p] = tr_replay_judge(window, a.recs[p].nonce, a.aead_status[p]);
    }
};

__global__ __launch_bounds__(TR_BLOCK) void tr_packet_commit(TrPacketArgs a)
{
    const uint32_t q = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (q >= a.count || !tr_run_head(a.keys, q, a.n)) return;
    tr_run_walk(a.keys, a.order, a.count, q, TrPacketJudge{a, a.replay + a.keys[q]});
}

/* a packet of a slot's run under the echo: judged as the open judges it, and an accepted one is made the
   seal's: the next send counter in front, its descriptor under that counter and the send context */
struct TrPacketEcho {
    const TrPacketArgs &a;
    TrReplay *window;
    uint64_t *send;              /* the lane's copy of the slot's */
    uint64_t ctx_off;
    TR_DEV void operator()(uint32_t p) const
    {
        uint64_t c;
        const uint8_t out = tr_echo_judge(window, send, a.recs[p].nonce, a.aead_status[p], &c);
        a.status[p] = out;
        /* a failed tag's descriptor is still the open's, live: nothing but an echoed packet may stay sealable */
        RecDesc d = refused_rec();
        if (!out) {
            const NoiseAeadPacket pk = a.packets[p];
            for (int b = 0; b < 8; ++b) a.wire[pk.off + b] = (uint8_t)(c >> (8 * b));
            d = tr_rec(pk.off + TR_COUNTER_LEN, c, ctx_off, pk.len - TR_DATAGRAM_MIN);
        }
        a.recs[p] = d;
    }
};

__global__ __launch_bounds__(TR_BLOCK) void tr_packet_echo(TrPacketArgs a)
{
    const uint32_t q = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (q >= a.count || !tr_run_head(a.keys, q, a.n)) return;
    const uint32_t i = a.keys[q];
    uint64_t send = a.send[i];
    tr_run_walk(a.keys, a.order, a.count, q, TrPacketEcho{a, a.replay + i, &send, (uint64_t)i * a.ctx_bytes});
    a.send[i] = send;
}

/* ---- keying and un-keying slots (section 10) */

struct TrKeyArgs {
    const uint32_t *slots;
    const uint8_t *k1, *k2;      /* tr_set_keys: entry j's keys at + 32 j */
    const uint8_t *status;       /* may be null; set: an entry whose byte is not 0 is cleared instead */
    uint8_t *ctx;                /* n send contexts, then n receive contexts */
    uint64_t *send, *recv;
    TrReplay *replay;
    uint8_t *keyed;
    uint64_t ctx_bytes;          /* a multiple of 16; the contexts are 16-byte aligned */
    uint32_t m, n;
    uint32_t set;                /* tr_clear_wide: 1 after gcm_prepare_slots (zero the failed, mark the rest keyed) */
    uint32_t initiator;
};

TR_DEV uint4 tr_load_key16(const uint8_t *p)
{
    uint32_t w[4];
    for (int q = 0; q < 4; ++q)
        w[q] = (uint32_t)p[4 * q] | ((uint32_t)p[4 * q + 1] << 8) | ((uint32_t)p[4 * q + 2] << 16) | ((uint32_t)p[4 * q + 3] << 24);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

/* both nonces, the anti-replay window and the state of slot i, shared among
   the caller's `lanes` lanes (lane 0 .. lanes - 1 each call it once) */
TR_DEV void tr_mark(const TrKeyArgs &a, uint32_t i, bool keyed, uint32_t lane = 0, uint32_t lanes = 1)
{
    uint64_t *window = (uint64_t *)(a.replay + i); /* top, then the bitmap */
    for (uint32_t q = lane; q < 1 + TR_REPLAY_WORDS; q += lanes) window[q] = 0;
    if (lane) return;
    a.send[i] = 0;
    a.recv[i] = 0;
    a.keyed[i] = keyed ? 1 : 0;
}

/* ChaChaPoly: the context is the key.  One lane per entry. */
__global__ __launch_bounds__(TR_BLOCK) void tr_set_keys(TrKeyArgs a)
{
    const uint32_t j = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (j >= a.m) return;
    uint32_t i;
    if (!tr_slot(a.slots, j, a.n, &i)) return;
    const bool failed = a.status && a.status[j];
    /* the initiator sends under k1 and receives under k2, the responder the other way round */
    const uint8_t *ks = (a.initiator ? a.k1 : a.k2) + (uint64_t)j * 32, *kr = (a.initiator ? a.k2 : a.k1) + (uint64_t)j * 32;
    uint4 *cs = (uint4 *)(a.ctx + (uint64_t)i * 32), *cr = (uint4 *)(a.ctx + ((uint64_t)a.n + i) * 32);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (int h = 0; h < 2; ++h) {
        cs[h] = failed ? zero : tr_load_key16(ks + 16 * h);
        cr[h] = failed ? zero : tr_load_key16(kr + 16 * h);
    }
    tr_mark(a, i, !failed);
}

/* contexts of at most a few 16-byte words: one lane per entry zeroes both */
__global__ __launch_bounds__(TR_BLOCK) void tr_clear_lane(TrKeyArgs a)
{
    const uint32_t j = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (j >= a.m) return;
    uint32_t i;
    if (!tr_slot(a.slots, j, a.n, &i)) return;
    const uint64_t words = a.ctx_bytes / 16;
    uint4 *cs = (uint4 *)(a.ctx + (uint64_t)i * a.ctx_bytes), *cr = (uint4 *)(a.ctx + ((uint64_t)a.n + i) * a.ctx_bytes);
    for (uint64_t w = 0; w < words; ++w) cs[w] = cr[w] = make_uint4(0, 0, 0, 0);
    tr_mark(a, i, false);
}

/* large contexts: one workgroup per (entry, direction), 2m in all.  With
   a.set, an entry that gcm_prepare_slots keyed is only marked. */
__global__ __launch_bounds__(TR_WIDE_BLOCK) void tr_clear_wide(TrKeyArgs a)
{
    const uint32_t j = blockIdx.x >> 1, receive = blockIdx.x & 1;
    if (j >= a.m) return;
    uint32_t i;
    if (!tr_slot(a.slots, j, a.n, &i)) return;
    const bool keep = a.set && !(a.status && a.status[j]);
    if (!receive && threadIdx.x < 1 + TR_REPLAY_WORDS) tr_mark(a, i, keep, threadIdx.x, 1 + TR_REPLAY_WORDS);
    if (keep) return;
    uint4 *c = (uint4 *)(a.ctx + ((uint64_t)receive * a.n + i) * a.ctx_bytes);
    for (uint64_t w = threadIdx.x, words = a.ctx_bytes / 16; w < words; w += TR_WIDE_BLOCK) c[w] = make_uint4(0, 0, 0, 0);
}

/* ---- rekey (section 12) */

/* REKEY(k) of the 32 key bytes at src, any alignment: bytes 0..31 of one
   ChaCha20 block (transport_plan.h TR_REKEY_CHACHA_*), all in registers;
   neither a branch nor an address depends on a key byte */
TR_DEV void tr_rekey_chacha(const uint8_t *src, uint32_t next[8])
{
    const uint4 lo = tr_load_key16(src), hi = tr_load_key16(src + 16);
    const uint32_t key[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t x[16];
    chacha20_block(key, TR_REKEY_CHACHA_COUNTER, 0, TR_REKEY_CHACHA_IV_LO, TR_REKEY_CHACHA_IV_HI, x);
#pragma unroll
    for (int w = 0; w < 8; ++w) next[w] = x[w];
}

/* raw keys: lane i turns the key at keys + 32 i into the one at out + 32 i
   (out may be keys: a lane reads its key before it writes) */
__global__ __launch_bounds__(TR_BLOCK) void tr_rekey_keys(const uint8_t *keys, uint8_t *out, uint32_t n)
{
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t next[8];
    tr_rekey_chacha(keys + (uint64_t)i * 32, next);
    uint8_t *o = out + (uint64_t)i * 32;
#pragma unroll
    for (int w = 0; w < 8; ++w)
        for (int b = 0; b < 4; ++b) o[4 * w + b] = (uint8_t)(next[w] >> (8 * b));
}

struct TrRekeyArgs {
    const uint32_t *slots;       /* may be null: entry j is slot j */
    const uint8_t *which;        /* may be null: every entry takes the call's directions */
    const uint8_t *keyed;
    uint8_t *ctx;                /* n send contexts, then n receive contexts */
    uint32_t m, n, directions;
};

/* the slots of an object, in place: one lane per (entry, direction), 2m in all */
__global__ __launch_bounds__(TR_BLOCK) void tr_rekey_slots(TrRekeyArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    const uint32_t receive = (uint32_t)t & 1;
    if (t >> 1 >= a.m) return;
    const uint32_t j = (uint32_t)(t >> 1);
    uint32_t i;
    if (!tr_slot(a.slots, j, a.n, &i) || !a.keyed[i]) return;
    if (!((tr_rekey_directions(a.directions, a.which, j) >> receive) & 1)) return;
    uint8_t *c = a.ctx + ((uint64_t)receive * a.n + i) * 32;
    uint32_t next[8];
    tr_rekey_chacha(c, next);
    ((uint4 *)c)[0] = make_uint4(next[0], next[1], next[2], next[3]);
    ((uint4 *)c)[1] = make_uint4(next[4], next[5], next[6], next[7]);
}

} // namespace

/* What the packet calls need for up to max_packets packets (section 13): a
   device allocation of its own beside the object's, made by _reserve_packets. */
struct TrPackets {
    DevArena dev;
    uint32_t max_packets;     /* 0: not reserved */
    uint32_t *keys[2], *order[2]; /* the sort's two buffers of each; a call starts in [0] */
    RecDesc *recs;
    uint8_t *status;          /* the AEAD's */
    void *sort_tmp;
    size_t sort_bytes;
};

struct NoiseAeadDevTransport {
    int cipher_id, role;
    uint32_t n, max_frames;
    size_t ctx_bytes;
    DevArena dev;             /* the one device allocation; the pointers below are its parts */
    uint8_t *ctx;            /* n send contexts, then n receive contexts */
    uint64_t *send, *recv, *count, *base;
    uint32_t *frames, *consumed;
    int32_t *stop;
    RecDesc *recs, *seal_recs;
    uint8_t *status;
    uint8_t *keyed;           /* per slot: 1 keyed, 0 not */
    TrReplay *replay;         /* per slot: the datagram calls' anti-replay window */
    void *scan_tmp;
    size_t scan_bytes;
    TrPackets packets;        /* what _reserve_packets made; all zero until then */
};

namespace {

typedef NoiseAeadDevTransport Tr;

/* the exclusive scan of the first m counts; tmp == nullptr asks for the size only */
int scan_counts(const Tr *tr, void *tmp, size_t &bytes, uint32_t m, hipStream_t s)
{
    return hip_rc(rocprim::exclusive_scan(tmp, bytes, (const uint64_t *)tr->count, tr->base, (uint64_t)0, (size_t)m,
                                          rocprim::plus<uint64_t>(), s));
}

/* One call over the m entries of `slots` (null: the n slots in order) under
   the cap max_frames (0: the object's); the arguments are checked.  d_result
   is the stream calls' and the datagram seal's, d_datagram_result and
   d_frame_status are the datagram open's. */
int run(Tr *tr, TrFraming framing, TrMode mode, const uint32_t *slots, uint32_t m, uint32_t max_frames, uint8_t *d_wire,
        const uint64_t *d_off, const uint32_t *d_len, NoiseAeadTransportResult *d_result,
        NoiseAeadDatagramResult *d_datagram_result, uint8_t *d_frame_status, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    size_t bytes = tr->scan_bytes;
    if (m != tr->n) { /* _new carved the scan's scratch for n items */
        size_t need = 0;
        const int rc1 = scan_counts(tr, nullptr, need, m, s);
        if (rc1) return rc1;
        if (need > tr->scan_bytes) return NOISE_ERROR_SYSTEM;
    }
    const bool datagram = framing == TR_DATAGRAM;
    const uint32_t cap = max_frames ? max_frames : tr->max_frames;
    const uint32_t most = m > cap ? m : cap; /* tr_build and an echo's tr_commit also pad the descriptors up to the cap */
    TrArgs a = {};
    a.wire = d_wire; a.off = d_off; a.len = d_len; a.result = d_result;
    a.send = tr->send; a.recv = tr->recv;
    a.count = tr->count; a.base = tr->base;
    a.frames = tr->frames; a.consumed = tr->consumed; a.stop = tr->stop;
    a.recs = tr->recs; a.seal_recs = tr->seal_recs; a.status = tr->status;
    a.ctx_bytes = tr->ctx_bytes; a.max_frames = cap;
    a.n = tr->n; a.mode = mode;
    a.slots = slots; a.keyed = tr->keyed; a.m = m;
    a.replay = datagram ? tr->replay : nullptr; /* a stream call has no window to touch */
    a.datagram_result = d_datagram_result; a.frame_status = d_frame_status;
    int rc = launch_items(datagram ? tr_count<TR_DATAGRAM> : tr_count<TR_STREAM>, m, TR_BLOCK, s, a);
    if (!rc) rc = scan_counts(tr, tr->scan_tmp, bytes, m, s);
    if (!rc) rc = launch_items(datagram ? tr_build<TR_DATAGRAM> : tr_build<TR_STREAM>, most, TR_BLOCK, s, a);
    if (rc) return rc;
    NoiseAeadRagged job = {};
    job.ctx_base = tr->ctx;
    job.recs = (const NoiseAeadRecord *)tr->recs;
    job.in = job.out = d_wire;
    job.ad = d_wire; /* never read: every ad_len is 0 */
    job.status = tr->status;
    job.n_records = cap;
    if (mode == TR_SEAL) return noise_aead_dev_seal_ragged(tr->cipher_id, &job, s);
    rc = noise_aead_dev_open_ragged(tr->cipher_id, &job, s);
    if (rc) return rc;
    if (datagram) return launch_items(tr_commit_datagrams, m, TR_BLOCK, s, a);
    rc = launch_items(tr_commit, mode == TR_ECHO ? most : m, TR_BLOCK, s, a);
    if (rc || mode == TR_OPEN) return rc;
    job.recs = (const NoiseAeadRecord *)tr->seal_recs;
    job.status = nullptr;
    return noise_aead_dev_seal_ragged(tr->cipher_id, &job, s);
}

/* the calls of section 9: every slot in order, the object's own cap */
int run_all(Tr *tr, TrMode mode, uint8_t *d_wire, const uint64_t *d_off, const uint32_t *d_len,
            NoiseAeadTransportResult *d_result, void *stream)
{
    const int rc = tr_check_call(tr, tr ? tr->n : 0, d_wire, d_off, d_len, d_result);
    if (rc || !tr->n) return rc;
    return run(tr, TR_STREAM, mode, nullptr, tr->n, 0, d_wire, d_off, d_len, d_result, nullptr, nullptr, stream);
}

/* the calls of section 10: the listed slots, the call's cap */
int run_of(Tr *tr, TrMode mode, const uint32_t *d_slots, uint32_t m, uint32_t max_frames, uint8_t *d_wire,
           const uint64_t *d_off, const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream)
{
    const int rc = tr_check_call_of(tr, tr ? tr->n : 0, tr ? tr->max_frames : 0, d_slots, m, max_frames, d_wire, d_off,
                                    d_len, d_result);
    if (rc || !m) return rc;
    return run(tr, TR_STREAM, mode, d_slots, m, max_frames, d_wire, d_off, d_len, d_result, nullptr, nullptr, stream);
}

/* the calls of section 11: the listed slots (null: entry j is slot j), the call's cap */
int run_datagrams(Tr *tr, TrMode mode, const uint32_t *d_slots, uint32_t m, uint32_t max_frames, uint8_t *d_wire,
                  const uint64_t *d_off, const uint32_t *d_len, NoiseAeadTransportResult *d_result,
                  NoiseAeadDatagramResult *d_datagram_result, uint8_t *d_frame_status, void *stream)
{
    const bool open = mode == TR_OPEN;
    const int rc = tr_check_datagrams(tr, tr ? tr->n : 0, tr ? tr->max_frames : 0, d_slots, m, max_frames, d_wire, d_off,
                                      d_len, open ? (const void *)d_datagram_result : (const void *)d_result,
                                      open ? sizeof(NoiseAeadDatagramResult) : sizeof(NoiseAeadTransportResult), open,
                                      d_frame_status);
    if (rc || !m) return rc;
    return run(tr, TR_DATAGRAM, mode, d_slots, m, max_frames, d_wire, d_off, d_len, d_result, d_datagram_result,
               d_frame_status, stream);
}

/* The stable sort of the first `count` (key, order) pairs over the low `bits`
   bits of the keys, from the buffers [0]; *keys and *order: where it leaves
   them.  tmp == nullptr asks for the size only, and nothing is launched. */
int sort_packets(const TrPackets &pk, void *tmp, size_t &bytes, uint32_t count, uint32_t bits, uint32_t **keys,
                 uint32_t **order, hipStream_t s)
{
    rocprim::double_buffer<uint32_t> k(pk.keys[0], pk.keys[1]), o(pk.order[0], pk.order[1]);
    const int rc = hip_rc(rocprim::radix_sort_pairs(tmp, bytes, k, o, (size_t)count, 0u, bits, s));
    *keys = k.current();
    *order = o.current();
    return rc;
}

/* The calls of sections 13 and 14: the packets of the list, one status byte
   each.  TR_ECHO is the open with tr_packet_echo in the commit's place, then
   the seal over the same descriptors. */
int run_packets(Tr *tr, TrMode mode, const NoiseAeadPacket *d_packets, uint32_t count, uint8_t *d_wire, uint8_t *d_status,
                void *stream)
{
    int rc = tr_check_packets(tr, tr ? tr->packets.max_packets : 0, d_packets, count, d_wire, d_status);
    if (rc || !count) return rc;
    hipStream_t s = (hipStream_t)stream;
    const TrPackets &pk = tr->packets;
    const uint32_t bits = tr_packet_key_bits(tr->n);
    TrPacketArgs a = {};
    size_t need = 0, bytes = pk.sort_bytes;
    rc = sort_packets(pk, nullptr, need, count, bits, &a.keys, &a.order, s); /* the size question: nothing is launched */
    if (rc) return rc;
    if (need > pk.sort_bytes) return NOISE_ERROR_SYSTEM;
    a.packets = d_packets; a.wire = d_wire; a.status = d_status;
    a.keys = pk.keys[0]; a.order = pk.order[0]; /* tr_packet_keys fills what the sort reads */
    a.recs = pk.recs; a.aead_status = pk.status;
    a.send = tr->send; a.replay = tr->replay; a.keyed = tr->keyed;
    a.ctx_bytes = tr->ctx_bytes;
    a.n = tr->n; a.count = count; a.mode = mode;
    rc = launch_items(tr_packet_keys, count, TR_BLOCK, s, a);
    if (!rc) rc = sort_packets(pk, pk.sort_tmp, bytes, count, bits, &a.keys, &a.order, s);
    if (!rc && mode == TR_SEAL) rc = launch_items(tr_packet_seal, count, TR_BLOCK, s, a);
    if (rc) return rc;
    NoiseAeadRagged job = {};
    job.ctx_base = tr->ctx;
    job.recs = (const NoiseAeadRecord *)pk.recs;
    job.in = job.out = d_wire;
    job.ad = d_wire; /* never read: every ad_len is 0 */
    job.status = pk.status;
    job.n_records = count;
    if (mode == TR_SEAL) return noise_aead_dev_seal_ragged(tr->cipher_id, &job, s);
    rc = noise_aead_dev_open_ragged(tr->cipher_id, &job, s);
    if (!rc) rc = launch_items(mode == TR_ECHO ? tr_packet_echo : tr_packet_commit, count, TR_BLOCK, s, a);
    if (rc || mode == TR_OPEN) return rc;
    job.status = nullptr; /* tr_packet_echo has written the caller's statuses */
    return noise_aead_dev_seal_ragged(tr->cipher_id, &job, s);
}

/* The object and its one device allocation, zeroed on s: every slot unkeyed,
   every nonce 0.  The arguments are checked. */
int make(Tr **out, int cipher_id, int role, uint32_t n, uint32_t max_frames, hipStream_t s)
{
    *out = nullptr;
    Tr *tr = new (std::nothrow) Tr();
    if (!tr) return NOISE_ERROR_NO_MEMORY;
    tr->cipher_id = cipher_id;
    tr->role = role;
    tr->n = n;
    tr->max_frames = max_frames;
    tr->ctx_bytes = noise_aead_dev_ctx_bytes(cipher_id);
    if (n) {
        int rc = scan_counts(tr, nullptr, tr->scan_bytes, n, s); /* the size question: nothing is launched */
        if (rc) {
            delete tr;
            return rc;
        }
        const size_t ns = n, nf = max_frames;
        DevArena &d = tr->dev;
        d.align = TR_ALIGN;
        const size_t o_ctx = d.carve(2 * ns * tr->ctx_bytes), o_send = d.carve(ns * 8), o_recv = d.carve(ns * 8);
        const size_t o_count = d.carve(ns * 8), o_base = d.carve(ns * 8), o_frames = d.carve(ns * 4);
        const size_t o_consumed = d.carve(ns * 4), o_stop = d.carve(ns * 4);
        const size_t o_recs = d.carve(nf * sizeof(RecDesc)), o_seal = d.carve(nf * sizeof(RecDesc));
        const size_t o_status = d.carve(nf), o_keyed = d.carve(ns), o_scan = d.carve(tr->scan_bytes);
        const size_t o_replay = d.carve(ns * sizeof(TrReplay));
        if (!d.alloc()) {
            delete tr;
            return NOISE_ERROR_NO_MEMORY;
        }
        tr->ctx = d.at(o_ctx); tr->send = d.at<uint64_t>(o_send); tr->recv = d.at<uint64_t>(o_recv);
        tr->count = d.at<uint64_t>(o_count); tr->base = d.at<uint64_t>(o_base);
        tr->frames = d.at<uint32_t>(o_frames); tr->consumed = d.at<uint32_t>(o_consumed);
        tr->stop = d.at<int32_t>(o_stop); tr->recs = d.at<RecDesc>(o_recs); tr->seal_recs = d.at<RecDesc>(o_seal);
        tr->status = d.at(o_status); tr->keyed = d.at(o_keyed); tr->scan_tmp = d.at(o_scan);
        tr->replay = d.at<TrReplay>(o_replay);
        rc = d.zero(s);
        if (rc) {
            noise_aead_dev_transport_free(tr);
            return rc;
        }
    }
    *out = tr;
    return NOISE_ERROR_NONE;
}

TrKeyArgs key_args(const Tr *tr, const uint32_t *d_slots, uint32_t m)
{
    TrKeyArgs a = {};
    a.slots = d_slots;
    a.ctx = tr->ctx;
    a.send = tr->send;
    a.recv = tr->recv;
    a.replay = tr->replay;
    a.keyed = tr->keyed;
    a.ctx_bytes = tr->ctx_bytes;
    a.m = m;
    a.n = tr->n;
    a.initiator = tr->role == NOISE_ROLE_INITIATOR;
    return a;
}

/* zero and un-key (set: after gcm_prepare_slots, the failed entries only; the rest are marked keyed) */
int launch_clear(const Tr *tr, const TrKeyArgs &a, hipStream_t s)
{
    if (tr->ctx_bytes <= 64) return launch_items(tr_clear_lane, a.m, TR_BLOCK, s, a);
    if (a.m > 0x7fffffffu / 2) return NOISE_ERROR_INVALID_PARAM; /* 2m workgroups in one grid */
    hipLaunchKernelGGL(tr_clear_wide, dim3(2 * a.m), dim3(TR_WIDE_BLOCK), 0, s, a);
    return hip_rc(hipGetLastError());
}

} // namespace

extern "C" {

int noise_aead_dev_transport_new(NoiseAeadDevTransport **out, int cipher_id, int role, uint32_t n, const uint8_t *d_k1,
                                 const uint8_t *d_k2, uint32_t max_frames, void *stream)
{
    int rc = tr_check_new(out, cipher_id, role, n, d_k1, d_k2, max_frames);
    if (rc) return rc;
    *out = nullptr;
    hipStream_t s = (hipStream_t)stream;
    Tr *tr = nullptr;
    rc = make(&tr, cipher_id, role, n, max_frames, s);
    if (rc) return rc;
    if (n) {
        /* every slot keyed; the initiator sends under k1, the responder under k2 */
        const bool init = role == NOISE_ROLE_INITIATOR;
        const size_t ns = n;
        rc = hip_rc(hipMemsetAsync(tr->keyed, 1, ns, s));
        if (!rc) rc = noise_aead_dev_prepare(cipher_id, init ? d_k1 : d_k2, n, tr->ctx, s);
        if (!rc) rc = noise_aead_dev_prepare(cipher_id, init ? d_k2 : d_k1, n, tr->ctx + ns * tr->ctx_bytes, s);
        if (rc) {
            noise_aead_dev_transport_free(tr);
            return rc;
        }
    }
    *out = tr;
    return NOISE_ERROR_NONE;
}

int noise_aead_dev_transport_new_unkeyed(NoiseAeadDevTransport **out, int cipher_id, int role, uint32_t n,
                                         uint32_t max_frames, void *stream)
{
    const int rc = tr_check_new_unkeyed(out, cipher_id, role, n, max_frames);
    if (rc) return rc;
    return make(out, cipher_id, role, n, max_frames, (hipStream_t)stream);
}

int noise_aead_dev_transport_set_keys(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m, const uint8_t *d_k1,
                                      const uint8_t *d_k2, const uint8_t *d_status, void *stream)
{
    int rc = tr_check_set_keys(tr, tr ? tr->n : 0, d_slots, m, d_k1, d_k2);
    if (rc || !m) return rc;
    hipStream_t s = (hipStream_t)stream;
    TrKeyArgs a = key_args(tr, d_slots, m);
    a.k1 = d_k1;
    a.k2 = d_k2;
    a.status = d_status;
    a.set = 1;
    if (tr->cipher_id == NOISE_CIPHER_CHACHAPOLY) return launch_items(tr_set_keys, m, TR_BLOCK, s, a);
    rc = aes_prepare_slots(d_slots, m, tr->n, d_k1, d_k2, d_status, a.initiator != 0, tr->ctx, s);
    return rc ? rc : launch_clear(tr, a, s);
}

int noise_aead_dev_transport_clear_keys(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m, void *stream)
{
    const int rc = tr_check_clear_keys(tr, tr ? tr->n : 0, d_slots, m);
    if (rc || !m) return rc;
    return launch_clear(tr, key_args(tr, d_slots, m), (hipStream_t)stream);
}

int noise_aead_dev_rekey(int cipher_id, const uint8_t *d_keys, uint32_t n, uint8_t *d_out, void *stream)
{
    const int rc = check_rekey(cipher_id, d_keys, n, d_out);
    if (rc || !n) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (cipher_id == NOISE_CIPHER_CHACHAPOLY) return launch_items(tr_rekey_keys, n, TR_BLOCK, s, d_keys, d_out, n);
    return aes_rekey_keys(d_keys, n, d_out, s);
}

int noise_aead_dev_transport_rekey(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m, uint32_t directions,
                                   const uint8_t *d_which, void *stream)
{
    const int rc = tr_check_rekey(tr, tr ? tr->n : 0, m, directions);
    if (rc || !m) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (tr->cipher_id != NOISE_CIPHER_CHACHAPOLY)
        return aes_rekey_slots(d_slots, m, tr->n, directions, d_which, tr->keyed, tr->ctx, s);
    const TrRekeyArgs a = {d_slots, d_which, tr->keyed, tr->ctx, m, tr->n, directions};
    return launch_items(tr_rekey_slots, 2 * (uint64_t)m, TR_BLOCK, s, a);
}

const uint8_t *noise_aead_dev_transport_has_key(const NoiseAeadDevTransport *tr)
{
    return tr ? tr->keyed : nullptr;
}

const uint8_t *noise_aead_debug_transport_ctx(const NoiseAeadDevTransport *tr, int direction, size_t *ctx_bytes)
{
    if (!tr || !tr->n || (direction != 0 && direction != 1)) return nullptr;
    if (ctx_bytes) *ctx_bytes = tr->ctx_bytes;
    return tr->ctx + (size_t)direction * tr->n * tr->ctx_bytes;
}

int noise_aead_dev_transport_free(NoiseAeadDevTransport *tr)
{
    if (!tr) return NOISE_ERROR_INVALID_PARAM;
    const int rc = tr->dev.release(), rc2 = tr->packets.dev.release();
    memset((void *)tr, 0, sizeof(*tr));
    delete tr;
    return rc ? rc : rc2;
}

int noise_aead_dev_transport_reserve_packets(NoiseAeadDevTransport *tr, uint32_t max_packets, void *stream)
{
    int rc = tr_check_reserve_packets(tr, max_packets, tr ? tr->packets.max_packets : 0);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    TrPackets pk = {};
    pk.max_packets = max_packets;
    /* the sort picks its algorithm by the count, and its scratch is not monotone in it: ask for every power
       of two up to max_packets and for max_packets itself, keep the most; a call still asks for its own count */
    for (uint64_t count = 1; count / 2 < max_packets; count *= 2) {
        uint32_t *unused;
        size_t need = 0;
        rc = sort_packets(pk, nullptr, need, count < max_packets ? (uint32_t)count : max_packets, tr_packet_key_bits(tr->n),
                          &unused, &unused, s);
        if (rc) return rc;
        if (need > pk.sort_bytes) pk.sort_bytes = need;
    }
    const size_t np = max_packets;
    DevArena &d = pk.dev;
    d.align = TR_ALIGN;
    const size_t o_keys0 = d.carve(np * 4), o_keys1 = d.carve(np * 4), o_order0 = d.carve(np * 4), o_order1 = d.carve(np * 4);
    const size_t o_recs = d.carve(np * sizeof(RecDesc)), o_status = d.carve(np), o_sort = d.carve(pk.sort_bytes);
    if (!d.alloc()) return NOISE_ERROR_NO_MEMORY;
    pk.keys[0] = d.at<uint32_t>(o_keys0); pk.keys[1] = d.at<uint32_t>(o_keys1);
    pk.order[0] = d.at<uint32_t>(o_order0); pk.order[1] = d.at<uint32_t>(o_order1);
    pk.recs = d.at<RecDesc>(o_recs); pk.status = d.at(o_status); pk.sort_tmp = d.at(o_sort);
    rc = d.zero(s);
    if (rc) {
        d.release();
        return rc;
    }
    tr->packets = pk;
    return NOISE_ERROR_NONE;
}

int noise_aead_dev_transport_seal_packets(NoiseAeadDevTransport *tr, const NoiseAeadPacket *d_packets, uint32_t count,
                                          uint8_t *d_wire, uint8_t *d_status, void *stream)
{
    return run_packets(tr, TR_SEAL, d_packets, count, d_wire, d_status, stream);
}

int noise_aead_dev_transport_open_packets(NoiseAeadDevTransport *tr, const NoiseAeadPacket *d_packets, uint32_t count,
                                          uint8_t *d_wire, uint8_t *d_status, void *stream)
{
    return run_packets(tr, TR_OPEN, d_packets, count, d_wire, d_status, stream);
}

int noise_aead_dev_transport_echo_packets(NoiseAeadDevTransport *tr, const NoiseAeadPacket *d_packets, uint32_t count,
                                          uint8_t *d_wire, uint8_t *d_status, void *stream)
{
    return run_packets(tr, TR_ECHO, d_packets, count, d_wire, d_status, stream);
}

uint64_t *noise_aead_dev_transport_nonces(const NoiseAeadDevTransport *tr, int direction)
{
    if (!tr || (direction != 0 && direction != 1)) return nullptr;
    return direction ? tr->recv : tr->send;
}

int noise_aead_dev_transport_seal_frames(NoiseAeadDevTransport *tr, uint8_t *d_wire, const uint64_t *d_off,
                                         const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream)
{
    return run_all(tr, TR_SEAL, d_wire, d_off, d_len, d_result, stream);
}

int noise_aead_dev_transport_open_frames(NoiseAeadDevTransport *tr, uint8_t *d_wire, const uint64_t *d_off,
                                         const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream)
{
    return run_all(tr, TR_OPEN, d_wire, d_off, d_len, d_result, stream);
}

int noise_aead_dev_transport_echo_frames(NoiseAeadDevTransport *tr, uint8_t *d_wire, const uint64_t *d_off,
                                         const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream)
{
    return run_all(tr, TR_ECHO, d_wire, d_off, d_len, d_result, stream);
}

int noise_aead_dev_transport_seal_frames_of(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m,
                                            uint32_t max_frames, uint8_t *d_wire, const uint64_t *d_off,
                                            const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream)
{
    return run_of(tr, TR_SEAL, d_slots, m, max_frames, d_wire, d_off, d_len, d_result, stream);
}

int noise_aead_dev_transport_open_frames_of(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m,
                                            uint32_t max_frames, uint8_t *d_wire, const uint64_t *d_off,
                                            const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream)
{
    return run_of(tr, TR_OPEN, d_slots, m, max_frames, d_wire, d_off, d_len, d_result, stream);
}

int noise_aead_dev_transport_echo_frames_of(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m,
                                            uint32_t max_frames, uint8_t *d_wire, const uint64_t *d_off,
                                            const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream)
{
    return run_of(tr, TR_ECHO, d_slots, m, max_frames, d_wire, d_off, d_len, d_result, stream);
}

int noise_aead_dev_transport_seal_datagrams(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m,
                                            uint32_t max_frames, uint8_t *d_wire, const uint64_t *d_off,
                                            const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream)
{
    return run_datagrams(tr, TR_SEAL, d_slots, m, max_frames, d_wire, d_off, d_len, d_result, nullptr, nullptr, stream);
}

int noise_aead_dev_transport_open_datagrams(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m,
                                            uint32_t max_frames, uint8_t *d_wire, const uint64_t *d_off,
                                            const uint32_t *d_len, NoiseAeadDatagramResult *d_result,
                                            uint8_t *d_frame_status, void *stream)
{
    return run_datagrams(tr, TR_OPEN, d_slots, m, max_frames, d_wire, d_off, d_len, nullptr, d_result, d_frame_status, stream);
}

uint64_t *noise_aead_dev_transport_replay(const NoiseAeadDevTransport *tr, uint32_t *bits)
{
    if (bits) *bits = TR_REPLAY_BITS;
    return tr && tr->n ? (uint64_t *)tr->replay : nullptr;
}

} // extern "C"
