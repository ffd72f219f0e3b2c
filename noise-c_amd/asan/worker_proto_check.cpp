/*
 * worker_proto_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd worker_proto_check; tests/test_worker_proto_host.py).
 *
 * The resident worker's request protocol (csrc/worker_proto.h) run on the
 * CPU under ASan/UBSan: the host's encode against the decode rules the
 * kernel applies, for both placements.  Every area (header chunks, stamped
 * chunks, raw tail, results, the caller's key / AD / record) is a heap block
 * of its exact size, so an overrun on either side is caught.
 *
 * Per case: request k is encoded over areas that hold request k - 1 (a
 * full-length one) in its scrubbed state, decoded chunk by chunk the way
 * aead_worker does, and compared with key || AD || zero pad || record
 * (|| tag) and the header's fields; a chunk or header chunk left at k - 1
 * must be judged stale, the poisoned header of an abandoned request must not
 * be servable, and the scrub must leave the stamps and nothing else.  (The
 * scrub rewrites the chunks its request used: they read k; the ones past
 * them keep the number they had, k - 1 here.)
 */
#include "../csrc/worker_proto.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace na;

static int g_fail;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++g_fail <= 20) {                                          \
                printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);      \
                printf(__VA_ARGS__);                                       \
                printf("\n");                                              \
            }                                                              \
        }                                                                  \
    } while (0)

template <typename T>
static T *exact(size_t bytes, size_t align = 16)
{
    /* aligned_alloc wants a multiple of the alignment; every aligned area is one */
    void *p = align > 1 ? aligned_alloc(align, bytes ? bytes : align) : malloc(bytes ? bytes : 1);
    if (!p) abort();
    return (T *)p;
}

struct Areas {
    bool vram;
    Placement p;
    uint32_t *req, *in;
    uint8_t *tail, *out, *buf;
    explicit Areas(bool v) : vram(v), p(placement(v))
    {
        req = exact<uint32_t>(worker_req_bytes(v));
        in = exact<uint32_t>(WORKER_IN_BYTES);
        tail = exact<uint8_t>(worker_tail_bytes(v), 1);
        out = exact<uint8_t>(WORKER_DATA, 1);
        buf = exact<uint8_t>(WORKER_DATA); /* the worker's LDS stream buffer */
        memset(req, 0, worker_req_bytes(v));
        memset(in, 0, WORKER_IN_BYTES);
        memset(tail, 0, worker_tail_bytes(v));
        memset(out, 0, WORKER_DATA);
    }
    ~Areas() { free(req); free(in); free(tail); free(out); free(buf); }
    Chunk chunk(const uint32_t *a, uint32_t t) const { return Chunk{a[4 * t], a[4 * t + 1], a[4 * t + 2], a[4 * t + 3]}; }
};

/* the kernel's header poll over the chunks it loaded: the request's number
   if the header is fresh (hdr filled), else `last` */
static bool header_fresh(const Areas &a, uint32_t last, uint32_t *hdr)
{
    const uint32_t s0 = hdr_seq(a.chunk(a.req, 0));
    bool fresh = s0 != last;
    for (uint32_t t = 0; t < a.p.hdr_chunks; ++t) {
        const Chunk c = a.chunk(a.req, t);
        fresh = fresh && hdr_stamped(a.vram, c, s0);
        hdr_unpack(a.vram, c, t, hdr);
    }
    return fresh;
}

/* the kernel's fetch: stamped chunks, then the raw tail; false if a chunk is stale */
static bool fetch_stream(const Areas &a, uint32_t seq, uint32_t total)
{
    const uint32_t n = stream_chunks(a.p, total);
    bool ok = true;
    for (uint32_t t = 0; t < n; ++t) {
        const Chunk v = a.chunk(a.in, t);
        if (!chunk_fresh(a.vram, v, seq)) ok = false;
        chunk_unpack(a.vram, v, t, a.buf);
    }
    if (stream_tail(a.p, total)) memcpy(a.buf + a.p.head, a.tail, stream_tail(a.p, total));
    return ok;
}

static uint8_t pattern(uint32_t i, uint32_t salt) { return (uint8_t)(1 + (i * 131u + salt * 29u + (i >> 8)) % 255u); } /* never 0 */

static void post(Areas &a, uint32_t k, const Request &r, const uint8_t *key, const uint8_t *ad, const uint8_t *data)
{
    encode_stream(a.vram, a.in, a.tail, k, key, ad, r.ad_len, data, r.len + (r.op ? 16u : 0u));
    encode_header(a.vram, a.req, k, r);
}

/* request k - 1 (the longest there is) posted, answered and scrubbed */
static void previous_request(Areas &a, uint32_t k1)
{
    static std::vector<uint8_t> big(WORKER_MAX_LEN + 16, 0xEE), ad(WORKER_MAX_AD, 0xDD), key(32, 0xCC);
    Request r = {};
    r.op = 1; r.len = WORKER_MAX_LEN; r.ad_len = WORKER_MAX_AD; r.cipher = 0x4301;
    post(a, k1, r, key.data(), ad.data(), big.data());
    memset(a.out, 0xAB, pad16(r.len + 16)); /* the worker's results */
    scrub_request(a.vram, a.in, a.tail, a.out, k1, r.op, r.len, r.ad_len);
}

static bool all_zero(const uint8_t *p, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (p[i]) return false;
    return true;
}

/* the stamped chunks in their scrubbed state: the first n stamped k, the rest
   stamped k_rest, no payload anywhere */
static bool scrubbed(const Areas &a, uint32_t n, uint32_t k, uint32_t k_rest)
{
    for (uint32_t t = 0; t < WORKER_SPEC; ++t) {
        const Chunk v = a.chunk(a.in, t);
        if (!chunk_fresh(a.vram, v, t < n ? k : k_rest)) return false;
        alignas(16) uint8_t pay[16] = {0};
        chunk_unpack(a.vram, v, 0, pay);
        if (!all_zero(pay, a.p.chunk_bytes)) return false;
    }
    return true;
}

static int run_case(bool vram, uint32_t op, uint32_t ad_len, uint32_t len, uint32_t k)
{
    Areas a(vram);
    const uint32_t k1 = k - 1, total = stream_total(op, len, ad_len), in_len = len + (op ? 16u : 0u);
    const int fail0 = g_fail;
    if (k1) previous_request(a, k1); /* number 0: the areas as set up */
    CHECK(scrubbed(a, WORKER_SPEC, k1, k1), "previous request not scrubbed");
    CHECK(all_zero(a.tail, worker_tail_bytes(vram)) && all_zero(a.out, WORKER_DATA), "previous tail / results");
    for (uint32_t t = 0; t < WORKER_SPEC; ++t)
        CHECK(!chunk_fresh(vram, a.chunk(a.in, t), k), "chunk %u of %u judged fresh for %u", t, k1, k);

    /* the caller's buffers, exact */
    uint8_t *key = exact<uint8_t>(32, 1), *ad = exact<uint8_t>(ad_len, 1), *data = exact<uint8_t>(in_len, 1);
    for (uint32_t i = 0; i < 32; ++i) key[i] = pattern(i, 1);
    for (uint32_t i = 0; i < ad_len; ++i) ad[i] = pattern(i, 2);
    for (uint32_t i = 0; i < in_len; ++i) data[i] = pattern(i, 3);
    Request r = {};
    r.op = op; r.ct = (k >> 3) & 1; r.len = len; r.ad_len = ad_len;
    r.nonce = 0xfedcba9876543210ull ^ k; r.cipher = 0x4301 + (k & 1);
    r.ctx = 0x00007f12345678a0ull + ((uint64_t)k << 4); r.gen = k * 2654435761u;
    const bool with_key = r.cipher == 0x4301;
    post(a, k, r, with_key ? key : nullptr, ad_len ? ad : nullptr, data);

    /* the worker's side */
    uint32_t hdr[16] = {0};
    CHECK(header_fresh(a, k1, hdr), "header of %u not fresh", k);
    CHECK(request_seq(hdr) == k, "seq");
    const Request g = request_of(hdr);
    CHECK(g.op == r.op && g.ct == r.ct && g.len == r.len && g.ad_len == r.ad_len && g.nonce == r.nonce &&
          g.cipher == r.cipher && g.ctx == r.ctx && g.gen == r.gen, "header fields");
    CHECK(stream_total(g.op, g.len, g.ad_len) == total, "total");
    memset(a.buf, 0x5A, WORKER_DATA);
    CHECK(fetch_stream(a, k, total), "a chunk of %u judged stale", k);
    {
        std::vector<uint8_t> want(total, 0);
        if (with_key) memcpy(want.data(), key, 32);
        if (ad_len) memcpy(want.data() + 32, ad, ad_len);
        if (in_len) memcpy(want.data() + 32 + pad16(ad_len), data, in_len);
        CHECK(memcmp(a.buf, want.data(), total) == 0, "stream bytes");
    }

    /* a stream chunk left at k - 1 (in device memory: either half) is stale */
    const uint32_t nch = stream_chunks(a.p, total);
    const uint32_t victims[3] = {0, nch / 2, nch - 1};
    for (uint32_t vi = 0; vi < 3; ++vi) {
        uint32_t *c = a.in + 4 * victims[vi];
        for (int word = 0; word < 4; ++word) {
            if (c[word] != k) continue; /* maybe a payload word equal to k: then still stale below or fresh both ways */
            const bool is_stamp = vram ? (word == 1 || word == 3) : word == 3;
            if (!is_stamp) continue;
            c[word] = k1;
            CHECK(!chunk_fresh(vram, a.chunk(a.in, victims[vi]), k), "stale chunk %u word %d taken", victims[vi], word);
            c[word] = k;
        }
    }
    /* a header with one chunk (one half) at k - 1 is not fresh */
    for (uint32_t t = 0; t < a.p.hdr_chunks; ++t)
        for (int word = 0; word < 4; word += 2) {
            if (!vram && word) continue;
            uint32_t h2[16], *c = a.req + 4 * t;
            c[word] = k1;
            CHECK(!header_fresh(a, k1, h2), "header chunk %u word %d at %u taken", t, word, k1);
            CHECK(!header_fresh(a, k1 - 1, h2), "header chunk %u word %d at %u taken (older last)", t, word, k1);
            c[word] = k;
        }
    {
        uint32_t h2[16];
        CHECK(header_fresh(a, k1, h2), "header restored");
    }

    /* the stop word is a chunk of its own, outside the header */
    CHECK(stop_word(vram, a.req) == a.req + 4 * a.p.stop_chunk && a.p.stop_chunk >= a.p.hdr_chunks, "stop chunk");
    *stop_word(vram, a.req) = 1;
    encode_header(vram, a.req, k, r);
    CHECK(stop_of(a.chunk(a.req, a.p.stop_chunk)) == 1, "a header cancelled the stop");
    *stop_word(vram, a.req) = 0;

    /* abandoned: not servable as k, and as k ^ 0x80000000 never whole */
    {
        std::vector<uint32_t> keep(a.req, a.req + worker_req_bytes(vram) / 4);
        uint32_t h2[16];
        poison_header(vram, a.req, k);
        CHECK(!header_fresh(a, k1, h2), "poisoned header taken");
        CHECK(hdr_seq(a.chunk(a.req, 0)) == (k ^ 0x80000000u), "poison number");
        bool whole = true;
        for (uint32_t t = 0; t < a.p.hdr_chunks; ++t) whole = whole && hdr_stamped(vram, a.chunk(a.req, t), k ^ 0x80000000u);
        CHECK(!whole, "poisoned header whole");
        const uint32_t lasts[4] = {0, k, k1, k ^ 0x80000000u};
        for (uint32_t last : lasts) CHECK(!header_fresh(a, last, h2), "poisoned header taken after %u", last);
        memcpy(a.req, keep.data(), worker_req_bytes(vram));
    }

    /* answered and scrubbed: the stamps stay, nothing else */
    memset(a.out, 0xAB, pad16(len + 16));
    scrub_request(vram, a.in, a.tail, a.out, k, op, len, ad_len);
    CHECK(scrubbed(a, nch, k, k1), "scrub: stamps / payload");
    CHECK(all_zero(a.tail, worker_tail_bytes(vram)), "scrub: tail");
    CHECK(all_zero(a.out, WORKER_DATA), "scrub: results");

    free(key); free(ad); free(data);
    if (g_fail != fail0) printf("  in case vram %d op %u ad %u len %u k %08x\n", (int)vram, op, ad_len, len, k);
    return g_fail != fail0;
}

int main()
{
    static_assert(placement(false).head == 3072 && placement(true).head == 2048, "heads");
    /* the poll: every lane's chunk lies inside the request area, lanes
       0..hdr_chunks read the header chunks in order and lane stop_chunk the
       stop word's chunk */
    for (int vram = 0; vram < 2; ++vram) {
        const Placement p = placement(vram != 0);
        uint32_t *area = exact<uint32_t>(worker_req_area(vram != 0));
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t *c = poll_chunk(vram != 0, area, lane);
            CHECK(c >= area && c + 4 <= area + worker_req_area(vram != 0) / 4, "poll_chunk lane %u", lane);
            if ((lane & 15) <= p.stop_chunk) CHECK(c == area + 4 * (lane & 15), "poll_chunk order lane %u", lane);
        }
        CHECK(poll_chunk(vram != 0, area, p.stop_chunk) == stop_word(vram != 0, area), "stop chunk polled");
        free(area);
    }
    const uint32_t ads[] = {0, 1, 16, 17, 255, 256};
    const uint32_t ks[] = {1u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    unsigned cases = 0, skipped = 0;
    for (int vram = 0; vram < 2; ++vram) {
        const Placement p = placement(vram != 0);
        for (uint32_t op = 0; op < 2; ++op)
            for (uint32_t ad_len : ads) {
                /* len 0 (a total of 32 with no AD, sealing), then the edges:
                   one chunk, the head, the longest record.  A chunk is
                   shorter than the key, so the one-chunk totals are always
                   skipped; they stay listed in case a chunk ever grows. */
                const uint32_t base = stream_total(op, 0, ad_len);
                const uint32_t totals[] = {base, p.chunk_bytes - 1, p.chunk_bytes, p.chunk_bytes + 1,
                                           p.head - 1, p.head, p.head + 1, p.head + 15, p.head + 16, p.head + 17,
                                           stream_total(op, 65519, ad_len)};
                for (uint32_t total : totals) {
                    if (total < base) { /* no len >= 0 gives it */
                        ++skipped;
                        continue;
                    }
                    for (uint32_t k : ks) {
                        run_case(vram != 0, op, ad_len, total - base, k);
                        ++cases;
                    }
                }
            }
    }
    printf("worker_proto_check: %u cases, %u totals skipped (no len >= 0), %d failures\n", cases, skipped, g_fail);
    return g_fail ? 1 : 0;
}
