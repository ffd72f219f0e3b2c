/*
 * worker_proto.h — the resident worker's request protocol, written once.
 *
 * How a single-record request travels from the calling thread (the encode
 * half: host only) to the worker's workgroup (the decode half: NA_HD, the
 * rules aead_worker applies to what it loaded) — and nothing else: no HIP
 * runtime call, no cipher.  Plain C++17, so the two halves are also checked
 * against each other on the CPU under ASan/UBSan (asan/worker_proto_check.cpp).
 * No other file knows where a byte sits in a chunk.
 *
 * The request's input stream is  key (32 B) || AD padded to 16 || record
 * [|| tag for open].  Its first `head` bytes are posted as 16-byte chunks
 * that each carry the request's sequence number — a chunk is its own proof of
 * freshness, so the worker reads chunk t speculatively with every poll of the
 * header (one round trip for header and data together), keeps the ones
 * stamped with the new number and re-reads only stale ones; the stream past
 * the head (records over ~3 KiB) is posted raw, written before the header
 * and read after it.
 *
 *                         host memory               device memory (vram)
 *   stream chunk          {b0, b1, b2, k}           {b0, k, b1, k}
 *   stream bytes / chunk  12                        8
 *   head (256 chunks)     3072                      2048
 *   header chunk          {k, A, B, C}  x 4         {k, A, k, B}, {k, C, k, 0}  x 4
 *   stop word             word 0 of chunk 4         word 0 of chunk 8
 *
 * Every chunk is written with one aligned 16-byte store.  In device memory
 * the CPU's stores go through write-combining buffers, which may write a
 * 16-byte store as two 8-byte pieces: there every 8-byte half carries the
 * number.  The worker takes a header only when all its chunks carry the
 * same new number: no torn header.  The stop word has a chunk of its own,
 * written only by park / stop / launch, never by a request's header (a
 * header written after a park used to carry stop = 0 and cancel it).
 */
#ifndef NA_WORKER_PROTO_H
#define NA_WORKER_PROTO_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <emmintrin.h>

#if defined(__HIPCC__)
#define NA_HD __host__ __device__ __forceinline__
#else
#define NA_HD inline
#endif

namespace na {

constexpr uint32_t WORKER_MAX_LEN = 65535 - 16; /* whole records only */
constexpr uint32_t WORKER_MAX_AD = 256;
/* data area: ChaCha key (32 B) || AD (padded to 16) || record || tag */
constexpr uint32_t WORKER_DATA = 32 + WORKER_MAX_AD + 65536 + 64;
constexpr uint32_t WORKER_SPEC = 256; /* chunks read with every poll: one per thread */
constexpr uint32_t WCHUNK_BYTES = 12; /* host memory: 12 stream bytes and the number */
constexpr uint32_t WORKER_HEAD = WORKER_SPEC * WCHUNK_BYTES; /* stream bytes sent as chunks */
constexpr uint32_t WORKER_TAIL = WORKER_DATA - WORKER_HEAD;  /* the rest, raw */
constexpr uint32_t VCHUNK_BYTES = 8;  /* device memory: {4 stream bytes, number} twice */
constexpr uint32_t VWORKER_HEAD = WORKER_SPEC * VCHUNK_BYTES;
constexpr uint32_t VWORKER_TAIL = WORKER_DATA - VWORKER_HEAD;
static_assert(WORKER_HEAD % 16 == 0 && VWORKER_HEAD % 16 == 0, "the raw tail lands 16-B aligned in LDS");

/* The request slot (host pinned, fine-grained): the request header in host
   memory (c0..c3), the stop chunk (c4), and — on their own 128-B line — the
   worker's words. */
struct alignas(128) WorkerSlot {
    /* host -> worker */
    uint32_t c0[4];    /* seq, op | ct << 8, len, ad_len */
    uint32_t c1[4];    /* seq, nonce lo, nonce hi, cipher */
    uint32_t c2[4];    /* seq, ctx lo, ctx hi, 0 */
    uint32_t c3[4];    /* seq, ctx generation, 0, 0 */
    uint32_t c4[4];    /* stop, 0, 0, 0 */
    uint8_t pad0[128 - 80];
    /* worker -> host */
    uint64_t done;     /* last request completed */
    uint32_t status;   /* 0 ok, 1 MAC failure, 2 input never arrived */
    uint32_t exiting;  /* the worker is leaving (or has left) */
    uint32_t stamps[8]; /* debug: s_memrealtime (10 ns) of the last request's phases */
    uint32_t fstamps[8]; /* debug: s_memtime (cycles) through the latency-first path */
    uint32_t leave[4];   /* debug: the last leave's born, now (10 ns ticks, low words), lifetime, gen */
    uint8_t pad1[128 - 96];
};
static_assert(sizeof(WorkerSlot) == 256, "slot layout");

/* Where the request sits decides its chunk format. */
struct Placement {
    uint32_t chunk_bytes; /* stream bytes per chunk */
    uint32_t head;        /* stream bytes sent as chunks */
    uint32_t hdr_chunks;  /* chunks of the request header */
    uint32_t stop_chunk;  /* the chunk whose word 0 is the stop word */
};
NA_HD constexpr Placement placement(bool vram)
{
    return vram ? Placement{VCHUNK_BYTES, VWORKER_HEAD, 8, 8} : Placement{WCHUNK_BYTES, WORKER_HEAD, 4, 4};
}
/* bytes of the request's areas: stamped chunks, raw tail (the worker reads
   it in 16-byte pieces), header chunks and stop chunk */
constexpr size_t WORKER_IN_BYTES = (size_t)WORKER_SPEC * 16;
constexpr size_t worker_tail_bytes(bool vram) { return WORKER_DATA - placement(vram).head; }
constexpr size_t worker_req_bytes(bool vram) { return 16 * ((size_t)placement(vram).stop_chunk + 1); }
/* The request area as the poll reads it: each lane of a row reads one chunk
   (poll_chunk), 8 of them in host memory — the slot's first 128-B line — and
   16 in device memory, where the stamped chunks follow it. */
constexpr size_t worker_req_area(bool vram) { return vram ? 256 : 128; }
static_assert(offsetof(WorkerSlot, done) == worker_req_area(false), "the worker's words start the second line");
static_assert(worker_req_bytes(false) <= worker_req_area(false) && worker_req_bytes(true) <= worker_req_area(true),
              "header and stop chunks inside the polled area");

/* What a request's header says: the four header fields' words, c0..c3 above
   without the number. */
struct Request {
    uint32_t op, ct;       /* 1 open; AES-GCM: constant-time GHASH */
    uint32_t len, ad_len;
    uint64_t nonce;
    uint32_t cipher;
    uint64_t ctx;          /* AES-GCM: device address of the context's pinned host copy */
    uint32_t gen;          /* and the generation it was written at */
};

#if defined(__HIPCC__)
using Chunk = uint4;
#else
struct Chunk { uint32_t x, y, z, w; };
#endif

NA_HD constexpr uint32_t pad16(uint32_t n) { return (n + 15) & ~15u; }

/* ------------------------------------------------------------ decode (NA_HD) */

/* the stream of (op, len, ad_len): its bytes, and how many of the stamped
   chunks hold them */
NA_HD constexpr uint32_t stream_total(uint32_t op, uint32_t len, uint32_t ad_len)
{
    return 32 + pad16(ad_len) + len + (op ? 16u : 0u);
}
NA_HD constexpr uint32_t stream_chunks(Placement p, uint32_t total)
{
    const uint32_t n = (total + p.chunk_bytes - 1) / p.chunk_bytes;
    return n < WORKER_SPEC ? n : WORKER_SPEC;
}
/* bytes of it that travel raw: tail[o] is stream byte p.head + o */
NA_HD constexpr uint32_t stream_tail(Placement p, uint32_t total) { return total > p.head ? total - p.head : 0u; }

/* is stream chunk v stamped seq (in device memory: both halves)? */
NA_HD bool chunk_fresh(bool vram, const Chunk &v, uint32_t seq) { return v.w == seq && (!vram || v.y == seq); }

/* stream chunk t's payload lands at stream byte chunk_bytes * t */
NA_HD void chunk_unpack(bool vram, const Chunk &v, uint32_t t, uint8_t *stream)
{
    uint32_t *d = (uint32_t *)(stream + placement(vram).chunk_bytes * t);
    if (vram) {
        d[0] = v.x; d[1] = v.z;
    } else {
        d[0] = v.x; d[1] = v.y; d[2] = v.z;
    }
}

/* the request-area chunk that lane `lane` of the polling wave reads: the
   header chunks, then the stop chunk (lanes past them re-read one: the same
   round trip) */
NA_HD const uint32_t *poll_chunk(bool vram, const uint32_t *req, uint32_t lane)
{
    return req + 4 * (lane & (uint32_t)(worker_req_area(vram) / 16 - 1));
}

/* header chunk c: the number it leads with (chunk 0's is the request's), and
   whether every stamp in it is s */
NA_HD uint32_t hdr_seq(const Chunk &c) { return c.x; }
NA_HD bool hdr_stamped(bool vram, const Chunk &c, uint32_t s) { return c.x == s && (!vram || c.z == s); }
/* the stop word, given chunk placement(vram).stop_chunk */
NA_HD uint32_t stop_of(const Chunk &c) { return c.x; }

/* header chunk t (< hdr_chunks) into hdr[16] = c0..c3 of WorkerSlot: host
   memory chunk k = {seq, A_k, B_k, C_k}; device memory chunk 2k = {seq, A_k,
   seq, B_k}, 2k + 1 = {seq, C_k, seq, 0} */
NA_HD void hdr_unpack(bool vram, const Chunk &c, uint32_t t, uint32_t *hdr)
{
    if (!vram) {
        hdr[4 * t] = c.x; hdr[4 * t + 1] = c.y; hdr[4 * t + 2] = c.z; hdr[4 * t + 3] = c.w;
    } else {
        const uint32_t k = t >> 1;
        if (t & 1) {
            hdr[4 * k + 3] = c.y;
        } else {
            hdr[4 * k] = c.x; hdr[4 * k + 1] = c.y; hdr[4 * k + 2] = c.w;
        }
    }
}
NA_HD uint32_t request_seq(const uint32_t *hdr) { return hdr[0]; }
NA_HD Request request_of(const uint32_t *hdr)
{
    Request r;
    r.op = hdr[1] & 0xff;
    r.ct = (hdr[1] >> 8) & 1;
    r.len = hdr[2];
    r.ad_len = hdr[3];
    r.nonce = (uint64_t)hdr[5] | ((uint64_t)hdr[6] << 32);
    r.cipher = hdr[7];
    r.ctx = (uint64_t)hdr[9] | ((uint64_t)hdr[10] << 32);
    r.gen = hdr[13];
    return r;
}

/* ------------------------------------------------------- encode (host only) */

/* 16-byte chunk store: one aligned SSE store, which the x86-64 hosts of
   MI355X (AVX-capable) perform atomically, so the worker never sees half of
   a chunk; the sequence number in every chunk catches a torn header */
inline void store_chunk(uint32_t *dst, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    _mm_store_si128((__m128i *)dst, _mm_set_epi32((int)d, (int)c, (int)b, (int)a));
}

/* a scrubbed stream chunk of request k: the stamps, no payload */
inline __m128i scrubbed_chunk(bool vram, uint32_t k)
{
    return vram ? _mm_set_epi32((int)k, 0, (int)k, 0) : _mm_set_epi32((int)k, 0, 0, 0);
}

/* Request k's input stream key || AD || pad || data[0, in_len) into the
   stamped chunks `in` (WORKER_IN_BYTES, 16-B aligned) and the raw `tail`
   (worker_tail_bytes); key may be null (AES-GCM: 32 zero bytes).  The caller
   orders it before the header (sfence). */
inline void encode_stream(bool vram, uint32_t *in, uint8_t *tail, uint32_t k, const uint8_t *key,
                          const uint8_t *ad, size_t ad_len, const uint8_t *data, size_t in_len)
{
    const Placement p = placement(vram);
    const size_t ad_pad = pad16((uint32_t)ad_len), total = 32 + ad_pad + in_len;
    const size_t head = total < p.head ? total : p.head;
    const size_t nchunks = (head + p.chunk_bytes - 1) / p.chunk_bytes;
    const __m128i keep = _mm_set_epi32(0, -1, -1, -1), stamp = scrubbed_chunk(false, k);
    const __m128i kk = _mm_set1_epi32((int)k);
    alignas(16) uint8_t tmp[WORKER_HEAD + 16];
    memset(tmp, 0, 32 + ad_pad);
    if (key) memcpy(tmp, key, 32);
    if (ad_len) memcpy(tmp + 32, ad, ad_len);
    if (head > 32 + ad_pad) memcpy(tmp + 32 + ad_pad, data, head - 32 - ad_pad);
    memset(tmp + head, 0, 16); /* the last chunk's bytes past the stream */
    if (vram) {
        for (size_t c = 0; c < nchunks; ++c) {
            const __m128i v = _mm_loadl_epi64((const __m128i *)(tmp + VCHUNK_BYTES * c));
            _mm_store_si128((__m128i *)(in + 4 * c), _mm_unpacklo_epi32(v, kk)); /* {b0, k, b1, k} */
        }
    } else {
        for (size_t c = 0; c < nchunks; ++c) {
            const __m128i v = _mm_loadu_si128((const __m128i *)(tmp + WCHUNK_BYTES * c));
            _mm_store_si128((__m128i *)(in + 4 * c), _mm_or_si128(_mm_and_si128(v, keep), stamp));
        }
    }
    explicit_bzero(tmp, head);
    if (total > head) memcpy(tail, data + (head - 32 - ad_pad), total - head);
}

/* Request k's header into `req` (worker_req_bytes; the stop chunk is left
   alone), after the stream. */
inline void encode_header(bool vram, uint32_t *req, uint32_t k, const Request &r)
{
    const uint32_t f[4][3] = {{r.op | r.ct << 8, r.len, r.ad_len},
                              {(uint32_t)r.nonce, (uint32_t)(r.nonce >> 32), r.cipher},
                              {(uint32_t)r.ctx, (uint32_t)(r.ctx >> 32), 0u},
                              {r.gen, 0u, 0u}};
    for (int c = 0; c < 4; ++c) {
        if (vram) { /* chunk 2c = {k, A, k, B}, 2c + 1 = {k, C, k, 0} */
            store_chunk(req + 8 * c, k, f[c][0], k, f[c][1]);
            store_chunk(req + 8 * c + 4, k, f[c][2], k, 0u);
        } else {
            store_chunk(req + 4 * c, k, f[c][0], f[c][1], f[c][2]);
        }
    }
}

/* The header of abandoned request k made unservable: its first chunk no
   longer agrees with the others, so a late workgroup cannot take it. */
inline void poison_header(bool vram, uint32_t *req, uint32_t k)
{
    const uint32_t bad = k ^ 0x80000000u;
    if (vram) store_chunk(req, bad, 0u, bad, 0u);
    else store_chunk(req, bad, 0u, 0u, 0u);
}

/* Request k is over: key, plaintext and results out of the shared memory.
   The stamps stay (a zeroed chunk would carry number 0, which no request
   has).  The worker writes its results in 16-B pieces: up to
   roundup16(len + 16). */
inline void scrub_request(bool vram, uint32_t *in, uint8_t *tail, uint8_t *out, uint32_t k, uint32_t op,
                          uint32_t len, uint32_t ad_len)
{
    const Placement p = placement(vram);
    const uint32_t total = stream_total(op, len, ad_len), nchunks = stream_chunks(p, total);
    const __m128i stamp = scrubbed_chunk(vram, k);
    for (uint32_t c = 0; c < nchunks; ++c) _mm_store_si128((__m128i *)(in + 4 * c), stamp);
    if (stream_tail(p, total)) explicit_bzero(tail, stream_tail(p, total));
    if (vram) _mm_sfence();
    explicit_bzero(out, pad16(len + 16));
}

/* the stop word: a chunk of its own, apart from the header the calls rewrite */
inline uint32_t *stop_word(bool vram, uint32_t *req) { return req + 4 * placement(vram).stop_chunk; }

} // namespace na

#endif
