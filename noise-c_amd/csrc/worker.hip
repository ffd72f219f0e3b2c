/*
 * worker.hip — the resident single-record engine of the CipherState calls.
 *
 * A per-record noise_cipherstate_encrypt/decrypt (src/protocol/cipherstate.c
 * :293-410, the call pattern of examples/echo) is one record of 1 B - 64 KiB.
 * Launching a kernel and waiting for it costs ~20 us on its own, 5x the
 * reference's whole ~4 us CPU call.  Instead, the first call on a device
 * starts resident workgroups (256 threads each) on private streams; each
 * polls a request slot and serves records as they are posted.  The request
 * (header and input stream) sits in fine-grained device memory that the CPU
 * writes through the BAR where the device has a large BAR, else in pinned
 * host memory; results, status and the done word always go to pinned host
 * memory, so each side polls memory of its own and writes the other's:
 *
 *   host (na_worker_crypt)                  worker (aead_worker)
 *   post: key || AD || record || tag
 *         as the request's stream,
 *         then its header, numbered k --->  poll:  sees a whole header with a
 *                                                  new number
 *                                           fetch: the stream (and the AES-GCM
 *                                                  context) into LDS
 *                                           run:   the record (the device code
 *                                                  of the ragged kernels, or
 *                                                  the latency-first engine)
 *   await: spins until done == k  <------   reply: results, status, fence,
 *                                                  done = k (release, system)
 *   collect_and_scrub: copies out,          scrub: the record out of LDS
 *         zeroes the shared memory
 *
 * The unit is three files:
 *   worker_proto.h   the request protocol, both halves side by side: slot
 *                    layout, chunk formats of the two placements, header,
 *                    stop word, poison, scrub (plain C++: also checked on
 *                    the CPU, asan/worker_proto_check.cpp)
 *   worker_chacha.h  the latency-first ChaChaPoly engine (worker_chacha_fast
 *                    for one-pass records, worker_chacha_multi past them)
 *   worker.hip       the kernel loop (aead_worker, one body: poll, fetch,
 *                    run, reply, scrub; AES-GCM records run aesgcm.hip's
 *                    gcm_wide_record) and the host driver (groups, launch /
 *                    park / recover, na_worker_crypt: claim_and_ensure, post,
 *                    await, collect_and_scrub)
 *
 * The worker exits on its own after IDLE of no requests (and after at most
 * LIFETIME), or when the host sets stop; every exit path is reached by every
 * thread of the workgroup (one barrier-synchronised loop).  Before leaving it
 * sets `exiting` and looks at the header once more, so a request posted
 * meanwhile is either served or seen by the host (exiting set, done behind):
 * the host then waits for the stream and starts the group again, which
 * resumes at the slot's `done`.
 *
 * Workers come in GROUPS: one kernel of S workgroups (request slots) on one
 * high-priority stream, so S calling threads share a hardware queue (a queue
 * runs nothing else while a resident kernel holds it).  A device runs one
 * group per high-priority queue but one (GPU_MAX_HW_QUEUES - 1: 3 by default,
 * the last left to the application), S = ceil(8 / groups) slots each (at most
 * WORKER_MAX_SLOTS = 4): 3 x 3 = 9 slots by default, one per calling thread
 * up to 9, each a workgroup on its own CU, claimed without waiting while one
 * is free.  A group leaves as a whole (aead_worker: the closing word), for
 * idleness only once all its slots are idle.  Batch launches that fill every
 * CU ask the resident groups to leave first (worker_park_for_batch), so no
 * batch workgroup waits for a worker's CU.
 *
 * Key material reaches the worker through the slot as well: the ChaCha key
 * itself, or for AES-GCM a pinned host copy of the state's device context
 * (made once per key).  A resident kernel never reads device memory that was
 * written after it started: another XCD's L2 would not be kept coherent with
 * its own, while host memory read after a system-scope acquire is always
 * current.
 *
 * Opens are two-pass (verify first, then decrypt): a rejected record's bytes
 * are never written back.  Records longer than WORKER_MAX_LEN, or any setup
 * failure, return NOISE_ERROR_NOT_APPLICABLE and the caller takes the
 * regular launch path.  NOISE_AEAD_WORKER=0 disables the worker.
 */
#include "launch.h"
#include "chachapoly.hip"
#define NA_NO_SETUP_KERNELS
#include "aesgcm.hip"
#include "worker_proto.h"
#include "worker_chacha.h"
#include <cstdlib>
#include <atomic>
#include <mutex>
#include <ctime>

namespace na {

/* AES-GCM contexts the worker keeps in LDS (an echo session uses two) */
constexpr int WORKER_CTX_SLOTS = 2;
constexpr uint32_t WORKER_CTX_BYTES = sizeof(AesCtx); /* rk, H, the H^1..H^4 and H^8 tables */

#define NA_SYS_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
#define NA_SYS_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM)

/* One 16-byte system-coherent load (a single request: the chunk is read
   whole, never half before and half after the host's 16-byte store). */
NA_DEV uint4 load_sys16(const uint32_t *p)
{
    uint4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=v"(v) : "v"(p) : "memory");
    return v;
}

/* two system-coherent 16-byte loads in one round trip */
NA_DEV void load_sys16x2(const uint32_t *p, const uint32_t *q, uint4 &a, uint4 &b)
{
    asm volatile("global_load_dwordx4 %0, %2, off sc0 sc1\n\t"
                 "global_load_dwordx4 %1, %3, off sc0 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b) : "v"(p), "v"(q) : "memory");
}

NA_DEV uint32_t now10ns() { return (uint32_t)__builtin_amdgcn_s_memrealtime(); }

/* 16 raw stream bytes, system-coherent, as two 8-byte atomic loads the
   compiler schedules (no wait per load) */
NA_DEV uint4 load_sys16_raw(const uint8_t *p)
{
    const uint64_t *q = (const uint64_t *)p;
    const uint64_t a = NA_SYS_LOAD(q), b = NA_SYS_LOAD(q + 1);
    return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
}

/* polls without a request after which only the header is polled: 20 us */
constexpr uint64_t POLL_BACKOFF = 2000;

/* A worker GROUP is one kernel of nslots workgroups on one high-priority
   stream, workgroup i serving request slot i: several calling threads per
   hardware queue (4 queues served at most 4 threads).  A group
   ends as a whole — a hardware queue runs nothing else until its kernel has
   left — so the workgroups agree on leaving through the group words (in the
   slots' placement, polled with the header in the same load instruction):
   word 0 `closing`, set by the first workgroup to leave (stop, idle,
   lifetime), after which every workgroup leaves between requests; words
   1..nslots the workgroups' last-request times.  A workgroup leaves for
   idleness only when every slot of the group has been idle that long.  Only
   the device writes the group words (`closing` is the number of the launch
   that closed, never reset by the host). */
constexpr int WORKER_MAX_SLOTS = 4;
struct WorkerSlotArgs {
    WorkerSlot *slot;      /* device view of the slot */
    const uint32_t *req;   /* the header chunks and the stop chunk */
    const uint4 *in;       /* the stream's stamped chunks */
    const uint8_t *tail;   /* the rest of the stream, raw */
    uint8_t *out;          /* results */
    uint32_t vram;
    uint32_t pad_;
};
struct WorkerArgs {
    WorkerSlotArgs s[WORKER_MAX_SLOTS];
    uint32_t *group;       /* the group words (8) */
    uint32_t nslots;
    uint32_t gen;          /* this launch's number: `closing` holds the number of the launch that closed */
    uint64_t idle, lifetime; /* s_memrealtime ticks (100 MHz) */
};

/* 256 threads per workgroup, one workgroup per slot. */
__global__ __launch_bounds__(256) void aead_worker(WorkerArgs a)
{
    const uint32_t me = blockIdx.x;
    WorkerSlot *const slot = a.s[me].slot;
    const uint32_t *const req = a.s[me].req;
    const uint4 *const in = a.s[me].in;
    const uint8_t *const tail = a.s[me].tail;
    uint8_t *const out = a.s[me].out;
    const uint32_t vram = a.s[me].vram;
    const uint64_t idle = a.idle, lifetime = a.lifetime;
    /* the last request served on this slot (a relaunched group starts where
       the one before it stopped: a request it left unserved is served) */
    uint32_t last = (uint32_t)NA_SYS_LOAD(&slot->done);
    const Placement p = placement(vram);
    __shared__ uint32_t te[256], sb[256];
    __shared__ __attribute__((aligned(16))) uint8_t cbuf[WORKER_CTX_SLOTS][WORKER_CTX_BYTES];
    __shared__ uint64_t ctag[WORKER_CTX_SLOTS]; /* host address of the cached context */
    __shared__ uint32_t cgen[WORKER_CTX_SLOTS], cuse[WORKER_CTX_SLOTS];
    __shared__ uint32_t hdr[16];
    __shared__ uint32_t s_cmd;          /* 0 wait, 1 serve, 2 leave */
    __shared__ uint32_t wl[40];         /* gcm_wide_record's verdict, E_K(J0), GHASH rows */
    __shared__ uint32_t s_stale;        /* chunks still stamped with an older request */
    __shared__ FastLds fast;
    __shared__ __attribute__((aligned(16))) uint8_t buf[WORKER_DATA];
    const uint32_t t = threadIdx.x;
    aes_table_entry(t, sb[t], te[t]);
    if (t < WORKER_CTX_SLOTS) {
        ctag[t] = 0;
        cgen[t] = 0;
        cuse[t] = 0;
    }
    const uint64_t born = __builtin_amdgcn_s_memrealtime();
    uint64_t quiet = born;
    /* the group word of this slot's last-request time is refreshed at most
       every idle / 8 (a system store the next poll would wait for: +0.7 us
       per call when written after every request); the idle test allows for
       the lag */
    uint64_t stamped = born;
    if (t == 0) NA_SYS_STORE(&a.group[1 + me], (uint32_t)born);
    bool leaving = false;
    uint32_t tick = 0;
    __shared__ uint32_t s_slow; /* backed-off polling (see below) */
    if (t == 0) s_slow = 0;
    __syncthreads();
    for (;;) {
        uint32_t t_seen = 0;
        /* every thread reads input chunk t; wave 0's lanes 0..3 (0..7 in
           device memory) hold the header (other lanes read a header chunk
           too: same round trip).  After POLL_BACKOFF without a request only
           wave 0 polls, the header alone (128 B instead of 8 KiB per poll:
           with the request in host memory every poll crosses PCIe), and a
           request then re-reads its chunks once (stamp 0 is never current).
           A wave may see the previous poll's setting: both are correct. */
        uint4 c = make_uint4(0, 0, 0, 0), mine = make_uint4(0, 0, 0, 0);
        /* lanes 14 and 15 of every 16 read the group words instead */
        const uint32_t *hp = (t & 15) >= 14 ? a.group + 4 * (t & 1) : poll_chunk(vram != 0, req, t);
        if (!s_slow) load_sys16x2(hp, (const uint32_t *)(in + t), c, mine);
        else if (t < 64) c = load_sys16(hp);
        if (t == 0) s_stale = 0;
        if (t < 64) {
            /* the header is taken when all its chunks carry one new number
               (worker_proto.h: 4 chunks in host memory, 8 in device memory) */
            const uint32_t s0 = __shfl((int)hdr_seq(c), 0, 64);
            uint32_t stop;
            bool fresh;
            if (!vram) {
                const uint32_t s1 = __shfl((int)hdr_seq(c), 1, 64);
                const uint32_t s2 = __shfl((int)hdr_seq(c), 2, 64), s3 = __shfl((int)hdr_seq(c), 3, 64);
                stop = __shfl((int)stop_of(c), (int)placement(false).stop_chunk, 64);
                fresh = s0 != last && s0 == s1 && s0 == s2 && s0 == s3;
                if (t < placement(false).hdr_chunks) hdr_unpack(false, c, t, hdr);
            } else {
                stop = __shfl((int)stop_of(c), (int)placement(true).stop_chunk, 64);
                fresh = s0 != last && __all(t >= placement(true).hdr_chunks || hdr_stamped(true, c, s0));
                if (t < placement(true).hdr_chunks) hdr_unpack(true, c, t, hdr);
            }
            /* the group words: closing, then the slots' last-request times */
            const bool closing = (uint32_t)__shfl((int)c.x, 14, 64) == a.gen;
            const uint32_t gq[WORKER_MAX_SLOTS] = {(uint32_t)__shfl((int)c.y, 14, 64),
                                                   (uint32_t)__shfl((int)c.z, 14, 64),
                                                   (uint32_t)__shfl((int)c.w, 14, 64),
                                                   (uint32_t)__shfl((int)c.x, 15, 64)};
            if (t == 0) {
                uint32_t cmd = 0;
                const uint64_t now = __builtin_amdgcn_s_memrealtime();
                bool group_idle = now - quiet > idle;
                for (uint32_t j = 0; j < a.nslots; ++j) /* 32-bit tick differences: idle < 2^31 */
                    if ((uint32_t)now - gq[j] <= (uint32_t)(idle + idle / 8)) group_idle = false;
                if (fresh) {
                    cmd = 1;
                } else if (leaving) {
                    cmd = 2;
                } else if (stop || closing || group_idle || now - born > lifetime) {
                    /* the group leaves with this workgroup; announce, then
                       poll once more: a request posted before that poll is
                       served; one posted after it finds `exiting` set and the
                       host starts the group again once all of it has left */
                    /* debug: why (stamps[7]: 1 stop, 2 closing, 4 idle, 8 lifetime) */
                    slot->stamps[7] = (stop ? 1u : 0u) | (closing ? 2u : 0u) | (group_idle ? 4u : 0u) |
                                      (now - born > lifetime ? 8u : 0u);
                    slot->leave[0] = (uint32_t)born;
                    slot->leave[1] = (uint32_t)now;
                    slot->leave[2] = (uint32_t)lifetime;
                    slot->leave[3] = a.gen;
                    NA_SYS_STORE(&a.group[0], a.gen);
                    NA_SYS_STORE(&slot->exiting, 1u);
                    leaving = true;
                } else if (now - quiet > POLL_BACKOFF) {
                    __builtin_amdgcn_s_sleep(8);
                } else {
                    __builtin_amdgcn_s_sleep(2);
                }
                s_slow = cmd == 0 && now - quiet > POLL_BACKOFF ? 1u : 0u;
                s_cmd = cmd;
                t_seen = (uint32_t)now;
            }
        }
        __syncthreads();
        const uint32_t cmd = s_cmd;
        if (cmd == 2) break;
        if (cmd == 0) {
            __syncthreads();
            continue;
        }
        /* serve request hdr[0]: the data area was written before the header;
           the acquire orders the reads below after the header's */
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        const uint32_t seq = request_seq(hdr);
        const Request rq = request_of(hdr);
        const uint32_t op = rq.op, ct = rq.ct, len = rq.len, ad_len = rq.ad_len, cipher = rq.cipher, gen = rq.gen;
        const uint64_t nonce = rq.nonce, ctx_addr = rq.ctx;
        const uint32_t ad_pad = pad16(ad_len);
        const uint32_t bytes = 32 + ad_pad + len + 16;
        const uint32_t t_fence = now10ns();
        /* the input stream: the head as stamped chunks (chunk t read
           speculatively with the poll, re-read while stale), the rest raw
           (written before the header, read after it).  Three rules of
           worker_proto.h are restated here, not called — stream_total (total),
           chunk_fresh (the stamp test) and chunk_unpack (d[]): calling them
           assembled differently from the text below, which is the measured
           one; asan/worker_proto_check.cpp checks the
           rules, so a change there must be made here too */
        const uint32_t total = 32 + ad_pad + len + (op ? 16u : 0u);
        const uint32_t nchunks = stream_chunks(p, total);
        if (t < nchunks) {
            uint4 v = mine;
            for (uint32_t tries = 0; (v.w != seq || (vram && v.y != seq)) && tries < (1u << 20); ++tries)
                v = load_sys16((const uint32_t *)(in + t));
            if (v.w != seq || (vram && v.y != seq)) s_stale = 1; /* never in practice: written before the header */
            uint32_t *d = (uint32_t *)(buf + p.chunk_bytes * t);
            if (vram) {
                d[0] = v.x; d[1] = v.z;
            } else {
                d[0] = v.x; d[1] = v.y; d[2] = v.z;
            }
        }
        for (uint32_t o = 16 * t; p.head + o < total; o += 16 * 256)
            *(uint4 *)(buf + p.head + o) = load_sys16_raw(tail + o);
        int cs = 0;
        if (cipher == NOISE_CIPHER_AESGCM) { /* the context: cached, or copied into the LRU slot */
            cs = ctag[0] == ctx_addr && cgen[0] == gen ? 0 : (ctag[1] == ctx_addr && cgen[1] == gen ? 1 : -1);
            if (cs < 0) {
                cs = cuse[0] <= cuse[1] ? 0 : 1;
                const uint8_t *src = (const uint8_t *)ctx_addr;
                for (uint32_t o = 16 * t; o < WORKER_CTX_BYTES; o += 16 * 256)
                    *(uint4 *)(cbuf[cs] + o) = *(const uint4 *)(src + o);
            }
        }
        __syncthreads();
        if (t == 0 && cipher == NOISE_CIPHER_AESGCM) {
            ctag[cs] = ctx_addr;
            cgen[cs] = gen;
            cuse[cs] = ++tick;
        }
        const uint32_t t_in = now10ns();
        if (t < 8) fast.dbg[t] = 0; /* the path's stamps: those it does not reach stay 0 */
        const uint64_t c_in = __builtin_amdgcn_s_memtime();
        uint8_t *key = buf, *ad = buf + 32, *rec = buf + 32 + ad_pad;
        bool ok = true;
        if (cipher == NOISE_CIPHER_CHACHAPOLY && worker_fast_fits(len, ad_len)) {
            ok = op ? worker_chacha_fast<true>(rec, ad, ad_len, len, key, nonce, fast)
                    : worker_chacha_fast<false>(rec, ad, ad_len, len, key, nonce, fast);
        } else if (cipher == NOISE_CIPHER_CHACHAPOLY) { /* past one pass */
            ok = op ? worker_chacha_multi<true>(rec, ad, ad_len, len, key, nonce, fast)
                    : worker_chacha_multi<false>(rec, ad, ad_len, len, key, nonce, fast);
        } else {
            const AesCtx *c = (const AesCtx *)cbuf[cs];
            const uint4 *h8 = (const uint4 *)c->tab8;
            if (ct) ok = op ? gcm_wide_record<true, true>(rec, rec, ad, ad_len, len, nonce, c, te, sb, h8, wl, nullptr, fast.dbg)
                            : gcm_wide_record<false, true>(rec, rec, ad, ad_len, len, nonce, c, te, sb, h8, wl, nullptr, fast.dbg);
            else ok = op ? gcm_wide_record<true, false>(rec, rec, ad, ad_len, len, nonce, c, te, sb, h8, wl, nullptr, fast.dbg)
                         : gcm_wide_record<false, false>(rec, rec, ad, ad_len, len, nonce, c, te, sb, h8, wl, nullptr, fast.dbg);
            if (t == 0) /* absolute s_memtime stamps -> cycles since c_in */
                for (int k = 0; k < 8; ++k) fast.dbg[k] = fast.dbg[k] ? fast.dbg[k] - (uint32_t)c_in : 0u;
        }
        __syncthreads();
        const uint32_t t_done = now10ns();
        const uint32_t c_run = (uint32_t)(__builtin_amdgcn_s_memtime() - c_in); /* shader cycles */
        /* results back: seal CT || tag, open the plaintext (only if verified);
           every storing wave drains its stores, then one system release and
           the flag (MI355X_MICROARCH.md, inter-workgroup visibility) */
        const bool stale = s_stale != 0;
        if (stale) ok = false;
        const uint32_t nout = op ? (ok ? len : 0u) : (stale ? 0u : len + 16);
        for (uint32_t o = 16 * t; o < ((nout + 15) & ~15u); o += 16 * 256)
            *(uint4 *)(out + o) = *(const uint4 *)(rec + o);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            const uint32_t t_out = now10ns();
            slot->status = stale ? 2u : (ok ? 0u : 1u);
            slot->stamps[0] = t_seen;
            slot->stamps[1] = t_fence;
            slot->stamps[2] = t_in;
            slot->stamps[3] = t_done;
            slot->stamps[4] = t_out;
            slot->stamps[6] = c_run;
            for (int k = 0; k < 8; ++k) slot->fstamps[k] = fast.dbg[k];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            slot->stamps[5] = now10ns();
            NA_SYS_STORE(&slot->done, (uint64_t)seq);
        }
        last = seq;
        quiet = __builtin_amdgcn_s_memrealtime();
        if (quiet - stamped > idle / 8) {
            if (t == 0) NA_SYS_STORE(&a.group[1 + me], (uint32_t)quiet);
            stamped = quiet;
        }
        /* scrub this record's bytes (and the key) from LDS before the next one;
           the kernels may have written whole 64-B units past len + 16 */
        for (uint32_t o = 16 * t; o < bytes + 64; o += 16 * 256) *(uint4 *)(buf + o) = make_uint4(0, 0, 0, 0);
        __syncthreads();
    }
    /* the cached AES-GCM contexts hold key material too */
    for (uint32_t o = 16 * t; o < WORKER_CTX_SLOTS * WORKER_CTX_BYTES; o += 16 * 256)
        *(uint4 *)(&cbuf[0][0] + o) = make_uint4(0, 0, 0, 0);
}

/* ------------------------------------------------------------- host side */

namespace {

struct WorkerGroup;

/* One request slot: served by one workgroup of its group's kernel. */
struct Worker {
    std::mutex mu;             /* held by the calling thread for a whole call */
    int state = 0;             /* 0 not set up, 1 usable, -1 failed */
    WorkerSlot *slot = nullptr; /* host view */
    WorkerSlot *dslot = nullptr; /* device view */
    /* the request (header chunks, stream): in fine-grained device memory the
       CPU writes through the BAR (vram), or in the host slot */
    bool vram = false;
    uint32_t *req = nullptr;    /* host view of the header chunks */
    const uint32_t *dreq = nullptr;
    void *vbase = nullptr;      /* the device allocation (vram) */
    uint4 *in = nullptr, *din = nullptr;       /* the stream's head: stamped chunks */
    uint8_t *tail = nullptr, *dtail = nullptr; /* the rest of the stream, raw */
    uint8_t *out = nullptr, *dout = nullptr;   /* raw results */
    uint32_t seq = 0;
    /* the AES-GCM contexts (host copies) sent to this slot's workgroup, whose
       LDS cache may hold them: only a group one of whose slots was sent a
       context is parked when the state is freed; past kCtxHist
       distinct ones since the group's launch, any free parks it */
    static constexpr int kCtxHist = 8;
    const void *ctx_hist[kCtxHist] = {};
    uint32_t ctx_n = 0;        /* written under mu (or at launch), read by forget() with atomics */
    WorkerGroup *g = nullptr;
};

/* One kernel on one high-priority stream: nslots workgroups, one per slot. */
struct WorkerGroup {
    std::mutex mu;             /* launch, drain, recover (taken after a slot's mu, never before) */
    int state = 0;             /* 0 unknown, 1 usable, -1 disabled, -2 draining (worker_abandon) */
    uint32_t launches = 0;     /* debug: kernels launched (noise_aead_debug_worker_launches) */
    int launch_fails = 0;      /* consecutive failed launches (3 disable the group) */
    hipStream_t stream = nullptr;
    bool launched = false;     /* written under mu, read by park() with atomics */
    uint32_t gen = 0;          /* launches so far (atomics): a relaunch happens once */
    uint32_t abandoned = 0;    /* slots whose request was abandoned: results scrubbed on recovery */
    uint32_t *words = nullptr; /* host view of the group words (8) */
    uint32_t *dwords = nullptr;
    bool words_vram = false;
    int nslots = 1;
    Worker slot[WORKER_MAX_SLOTS];
};

constexpr int kMaxDev = 64;
constexpr int kMaxGroups = 8;

/* The environment switches: each read once, by its getter's static
   (dispatch.h env_flag / env_int / env_choice). */

/* A resident group never ends while calls keep coming (up to LIFETIME), so
   it must own its hardware queue: a kernel queued behind it on the same AQL
   queue waits for it to leave.  HIP maps streams onto GPU_MAX_HW_QUEUES
   queues per device and priority (4 by default), so the groups run on
   high-priority streams — a pool apart from the application's normal
   streams (tools/queue_probe.cpp: a memset on a new normal stream waited
   the worker's whole 5 s lifetime beside a normal-priority worker, 20-60 us
   beside high-priority ones) — and a device runs one group per queue of that
   pool but one: the last queue stays free for a high-priority stream of the
   application's own.  NOISE_AEAD_WORKER_QUEUES sets the number
   of queues the groups take instead (1..8; an application with several
   high-priority streams of its own lowers it, or raises GPU_MAX_HW_QUEUES).
   NOISE_AEAD_WORKER_PRIO=normal / low: the A/B placements. */
int worker_stream_prio()
{
    static const int v = 1 - env_choice("NOISE_AEAD_WORKER_PRIO", {"normal", "low"}); /* high 1, normal 0, low -1 */
    return v;
}

int groups_per_dev()
{
    static const int v = [] {
        const int q = env_int("GPU_MAX_HW_QUEUES", 4);
        const int g = env_int("NOISE_AEAD_WORKER_QUEUES", q > 1 ? q - 1 : 1);
        return g < kMaxGroups ? g : kMaxGroups;
    }();
    return v;
}

/* Slots per group: enough for 8 calling threads over the groups
   (NOISE_AEAD_WORKER_SLOTS: 1..4).  A CipherState is single-owner with no
   locks (cipherstate.c:293-410), so N threads on N states run N calls at once
   on the CPU; here each calling thread gets a slot of its own (a workgroup on
   its own CU), claimed without waiting while one is free. */
int slots_per_group()
{
    static const int v = [] {
        const int s = env_int("NOISE_AEAD_WORKER_SLOTS", (8 + groups_per_dev() - 1) / groups_per_dev());
        return s < WORKER_MAX_SLOTS ? s : WORKER_MAX_SLOTS;
    }();
    return v;
}

WorkerGroup g_group[kMaxDev][kMaxGroups];
std::atomic<uint32_t> g_next_pref{0};
thread_local int t_pref = -1;             /* this thread's first-choice slot (spread over groups first) */
thread_local Worker *t_last = nullptr;    /* the slot of this thread's last call (debug hooks) */
std::once_flag g_atexit_once;

constexpr uint64_t IDLE_TICKS = 200000;       /* 2 ms at 100 MHz */
/* Test hook: NOISE_AEAD_DEBUG_WORKER_IDLE_MS overrides the idle timeout. */
uint64_t idle_ticks()
{
    static const int ms = env_int("NOISE_AEAD_DEBUG_WORKER_IDLE_MS", 0);
    return ms ? (uint64_t)ms * 100000ull : IDLE_TICKS;
}
constexpr uint64_t LIFETIME_TICKS = 500000000; /* 5 s */
/* The longest request (a 65519-B AES-GCM record) takes ~0.4 ms; a group
   that has not answered after this is taken for lost: the call falls back to
   the launch path and the group is drained before it is used again. */
constexpr uint64_t WAIT_LIMIT_NS = 2000000000ull; /* 2 s */

void set_stops(WorkerGroup &g, uint32_t v)
{
    for (int i = 0; i < g.nslots; ++i)
        if (g.slot[i].state == 1) __atomic_store_n(stop_word(g.slot[i].vram, g.slot[i].req), v, __ATOMIC_RELEASE);
    _mm_sfence();
}

/* Ask a launched group to leave (no wait).  A workgroup leaving scrubs its
   LDS; a request racing with the stop is either served or seen by its caller
   as `exiting` (the caller then starts the group again).  The stop words
   have chunks of their own, so no request header written meanwhile can undo
   them. */
void park_group(WorkerGroup &g)
{
    if (__atomic_load_n(&g.launched, __ATOMIC_ACQUIRE)) set_stops(g, 1u);
}

void park_device(int dev)
{
    for (int i = 0; i < kMaxGroups; ++i) park_group(g_group[dev][i]);
}

/* Did slot w (maybe) receive AES-GCM context h since its group's launch? */
bool worker_saw_ctx(const Worker &w, const void *h)
{
    const uint32_t n = __atomic_load_n(&w.ctx_n, __ATOMIC_ACQUIRE);
    if (n > (uint32_t)Worker::kCtxHist) return true; /* history overflowed */
    for (uint32_t i = 0; i < n; ++i)
        if (__atomic_load_n(&w.ctx_hist[i], __ATOMIC_RELAXED) == h) return true;
    return false;
}

/* (under w.mu) record that context h goes to slot w */
void worker_note_ctx(Worker &w, const void *h)
{
    const uint32_t n = w.ctx_n;
    if (n > (uint32_t)Worker::kCtxHist) return;
    for (uint32_t i = 0; i < n; ++i)
        if (w.ctx_hist[i] == h) return;
    if (n < (uint32_t)Worker::kCtxHist) __atomic_store_n(&w.ctx_hist[n], h, __ATOMIC_RELAXED);
    __atomic_store_n(&w.ctx_n, n + 1, __ATOMIC_RELEASE);
}

/* A request the group did not answer within WAIT_LIMIT_NS (under w.mu): the
   group is asked to leave and the request's header is made unservable — its
   first chunk no longer agrees with the others — so a late workgroup cannot
   take it; the group is drained (state -2) and made usable again once its
   stream is idle (worker_recover), when the slot's result area is scrubbed
   once more in case a late workgroup wrote it. */
void worker_abandon(Worker &w, uint32_t k)
{
    WorkerGroup &g = *w.g;
    /* the stop words and this slot's header first, without the group's
       lock: a caller holding it may be waiting in group_launch for this very
       group to leave */
    set_stops(g, 1u);
    poison_header(w.vram, w.req, k);
    _mm_sfence();
    std::lock_guard<std::mutex> gl(g.mu);
    g.abandoned |= 1u << (int)(&w - g.slot);
    g.state = -2;
}

/* (under g.mu, the group's stream idle) the result areas of the slots whose
   request was abandoned, in case a late workgroup wrote them */
void scrub_abandoned(WorkerGroup &g)
{
    for (int i = 0; i < g.nslots; ++i)
        if (g.abandoned & (1u << i)) explicit_bzero(g.slot[i].out, WORKER_DATA);
}

/* (under g.mu) a drained group whose stream has gone idle: the abandoned
   slots' results scrubbed, usable again (relaunched by the next call) */
void worker_recover(WorkerGroup &g)
{
    if (g.state != -2 || hipStreamQuery(g.stream) != hipSuccess) return;
    scrub_abandoned(g);
    g.abandoned = 0;
    __atomic_store_n(&g.launched, false, __ATOMIC_RELEASE);
    g.state = 1;
}

void worker_stop_all()
{
    for (int d = 0; d < kMaxDev; ++d)
        for (int i = 0; i < kMaxGroups; ++i) {
            WorkerGroup &g = g_group[d][i];
            std::lock_guard<std::mutex> lk(g.mu);
            if ((g.state != 1 && g.state != -2) || !g.launched) continue;
            set_stops(g, 1u);
            (void)hipStreamSynchronize(g.stream);
            scrub_abandoned(g);
            __atomic_store_n(&g.launched, false, __ATOMIC_RELEASE);
        }
}

bool worker_enabled()
{
    static const bool v = env_flag("NOISE_AEAD_WORKER", true);
    return v;
}

/* The request goes to device memory when the CPU can store to it (a large
   BAR: hipDeviceAttributeIsLargeBar): the worker then polls its own HBM and
   the host's stores arrive as posted PCIe writes, ordered behind each other
   (tools/microbench/doorbell.hip: 1 KiB request + doorbell -> acknowledgement
   3.2 us vs 4.9-5.5 us polling host memory).  NOISE_AEAD_WORKER_VRAM=0 keeps
   it in host memory. */
bool vram_wanted(int dev)
{
    if (!env_flag("NOISE_AEAD_WORKER_VRAM", true)) return false;
    int large_bar = 0;
    return hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, dev) == hipSuccess && large_bar;
}

int slot_setup(Worker &w, int dev)
{
    if (w.state) return w.state;
    w.state = -1;
    /* the worker reads the raw tail in 16-byte pieces: 64 bytes of slack */
    const size_t in_bytes = WORKER_IN_BYTES, tail_bytes = worker_tail_bytes(false) + 64;
    const size_t total = sizeof(WorkerSlot) + in_bytes + tail_bytes + WORKER_DATA;
    if (hipHostMalloc((void **)&w.slot, total, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
        return -1;
    memset(w.slot, 0, total); /* chunk stamps 0: no request has that number */
    if (hipHostGetDevicePointer((void **)&w.dslot, w.slot, 0) != hipSuccess) return -1;
    w.in = (uint4 *)(w.slot + 1);
    w.din = (uint4 *)(w.dslot + 1);
    w.tail = (uint8_t *)(w.in + WORKER_SPEC);
    w.dtail = (uint8_t *)(w.din + WORKER_SPEC);
    w.out = w.tail + tail_bytes;
    w.dout = w.dtail + tail_bytes;
    w.req = w.slot->c0;
    w.dreq = w.dslot->c0;
    /* device-memory request: the polled request area (worker_proto.h), the
       stamped chunks, then the raw tail */
    const size_t vbytes = worker_req_area(true) + in_bytes + worker_tail_bytes(true) + 64;
    if (vram_wanted(dev) && hipExtMallocWithFlags(&w.vbase, vbytes, hipDeviceMallocFinegrained) == hipSuccess) {
        memset(w.vbase, 0, vbytes); /* through the BAR mapping */
        _mm_sfence();
        w.vram = true;
        w.req = (uint32_t *)w.vbase;
        w.dreq = (const uint32_t *)w.vbase;
        w.in = w.din = (uint4 *)((uint8_t *)w.vbase + worker_req_area(true));
        w.tail = w.dtail = (uint8_t *)(w.in + WORKER_SPEC);
    }
    w.state = 1;
    return 1;
}

/* (under g.mu) the group's stream, words and slots, once */
int group_setup(WorkerGroup &g, int dev)
{
    if (g.state) return g.state;
    g.state = -1;
    g.nslots = slots_per_group();
    for (int i = 0; i < g.nslots; ++i) {
        g.slot[i].g = &g;
        if (slot_setup(g.slot[i], dev) != 1) return -1;
    }
    void *vw = nullptr;
    if (g.slot[0].vram && hipExtMallocWithFlags(&vw, 256, hipDeviceMallocFinegrained) == hipSuccess) {
        memset(vw, 0, 256);
        _mm_sfence();
        g.words = g.dwords = (uint32_t *)vw;
        g.words_vram = true;
    } else {
        if (hipHostMalloc((void **)&g.words, 256, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
            return -1;
        memset(g.words, 0, 256);
        if (hipHostGetDevicePointer((void **)&g.dwords, g.words, 0) != hipSuccess) return -1;
    }
    if (worker_stream_prio() == 0) {
        if (hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking) != hipSuccess) return -1;
    } else {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return -1;
        if (hipStreamCreateWithPriority(&g.stream, hipStreamNonBlocking,
                                        worker_stream_prio() > 0 ? greatest : least) != hipSuccess)
            return -1;
    }
    std::call_once(g_atexit_once, [] { atexit(worker_stop_all); });
    g.state = 1;
    return 1;
}

/* NOISE_ERROR_NONE, or NOISE_ERROR_NOT_APPLICABLE (the caller takes the
   launch path; three failures in a row retire the group) */
/* Test hook: NOISE_AEAD_DEBUG_WORKER_FAIL=1 makes every worker launch fail
   (tests/test_gpu_worker.py: the calls must then take the launch path). */
bool debug_launch_fails()
{
    static const bool v = env_flag("NOISE_AEAD_DEBUG_WORKER_FAIL", false);
    return v;
}

/* Test hook: NOISE_AEAD_DEBUG_WORKER_LEAVE=1 makes the group leave after a
   call has checked it is up and before it posts its request, so the wait
   loop must relaunch it (the mid-wait relaunch of ADVICE r5,
   tests/worker_mode_check.py --relaunch-free). */
bool debug_leave_before_post()
{
    static const bool v = env_flag("NOISE_AEAD_DEBUG_WORKER_LEAVE", false);
    return v;
}

/* NOISE_AEAD_WORKER_PARK=0: batch launches leave the workers resident (the
   A/B of tests/test_gpu_worker.py's batch-beside-worker measurement). */
bool park_enabled()
{
    static const bool v = env_flag("NOISE_AEAD_WORKER_PARK", true);
    return v;
}

/* (under g.mu, by the caller of slot `own`, whose mu it holds) start the
   group once the kernel before it has left: every slot's exiting and stop
   cleared, the closing word cleared.  Each workgroup starts at its slot's
   `done`, so a request a leaving group did not take is served now. */
int group_launch(WorkerGroup &g, Worker &own)
{
    (void)hipStreamSynchronize(g.stream); /* the kernel before has left (all its workgroups) */
    if (debug_launch_fails()) {
        if (++g.launch_fails >= 3) g.state = -1;
        return NOISE_ERROR_NOT_APPLICABLE;
    }
    WorkerArgs a = {};
    for (int i = 0; i < g.nslots; ++i) {
        Worker &w = g.slot[i];
        __atomic_store_n(&w.slot->exiting, 0u, __ATOMIC_RELEASE);
        __atomic_store_n(stop_word(w.vram, w.req), 0u, __ATOMIC_RELEASE);
        /* a fresh group caches nothing: the history restarts for slots not
           in a call (a slot in a call may be noting a context right now) */
        if (&w == &own) {
            __atomic_store_n(&w.ctx_n, 0u, __ATOMIC_RELEASE);
        } else {
            std::unique_lock<std::mutex> l(w.mu, std::try_to_lock);
            if (l.owns_lock()) __atomic_store_n(&w.ctx_n, 0u, __ATOMIC_RELEASE);
        }
        a.s[i].slot = w.dslot;
        a.s[i].req = w.dreq;
        a.s[i].in = (const uint4 *)w.din;
        a.s[i].tail = (const uint8_t *)w.dtail;
        a.s[i].out = w.dout;
        a.s[i].vram = w.vram ? 1u : 0u;
    }
    _mm_sfence();
    a.group = g.dwords;
    a.gen = __atomic_load_n(&g.gen, __ATOMIC_RELAXED) + 1u; /* never 0: the words start zeroed */
    a.nslots = (uint32_t)g.nslots;
    a.idle = idle_ticks();
    a.lifetime = LIFETIME_TICKS;
    hipLaunchKernelGGL(aead_worker, dim3(g.nslots), dim3(256), 0, g.stream, a);
    if (hipGetLastError() != hipSuccess) {
        if (++g.launch_fails >= 3) g.state = -1;
        return NOISE_ERROR_NOT_APPLICABLE;
    }
    g.launch_fails = 0;
    __atomic_add_fetch(&g.launches, 1u, __ATOMIC_RELAXED);
    __atomic_store_n(&g.launched, true, __ATOMIC_RELEASE);
    __atomic_add_fetch(&g.gen, 1u, __ATOMIC_RELEASE);
    return NOISE_ERROR_NONE;
}

/* (by the caller of slot w, holding w.mu) make sure w's group runs: gen0 is
   the group generation read BEFORE the caller saw it gone or leaving; if a
   relaunch happened since, there is nothing to do. */
std::atomic<uint32_t> g_dbg_ensure[4]; /* debug: group_ensure calls by cause (0 not launched, 1 exiting at the
                                          call, 2 exiting while waiting), 3 of them launched nothing */

int group_ensure(Worker &w, uint32_t gen0, int cause)
{
    WorkerGroup &g = *w.g;
    std::lock_guard<std::mutex> gl(g.mu);
    g_dbg_ensure[cause].fetch_add(1, std::memory_order_relaxed);
    if (g.state != 1) return NOISE_ERROR_NOT_APPLICABLE;
    if (__atomic_load_n(&g.gen, __ATOMIC_ACQUIRE) != gen0 && __atomic_load_n(&g.launched, __ATOMIC_ACQUIRE)) {
        g_dbg_ensure[3].fetch_add(1, std::memory_order_relaxed);
        return NOISE_ERROR_NONE;
    }
    return group_launch(g, w);
}

/* (holding w.mu) is w's group usable: recovered if drained, set up once */
bool group_usable(Worker &w, WorkerGroup &g, int dev)
{
    std::lock_guard<std::mutex> gl(g.mu);
    worker_recover(g);
    (void)w;
    return group_setup(g, dev) == 1;
}

/* slot n of the device's flattened order: spread over the groups first */
Worker &slot_n(int dev, int n)
{
    const int ng = groups_per_dev(), ns = slots_per_group();
    n %= ng * ns;
    WorkerGroup &g = g_group[dev][n % ng];
    return g.slot[(n / ng) % ns];
}

/* A usable slot of device dev, locked: this thread's own if free, else the
   first free one, else wait for this thread's own.  nullptr: none usable
   (set up failed on all of them). */
Worker *claim_worker(int dev, std::unique_lock<std::mutex> &lk)
{
    const int ng = groups_per_dev(), nw = ng * slots_per_group();
    if (t_pref < 0) t_pref = (int)(g_next_pref.fetch_add(1, std::memory_order_relaxed) % (uint32_t)nw);
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < nw; ++i) {
            const int n = (t_pref + i) % nw;
            WorkerGroup &g = g_group[dev][n % ng];
            Worker &w = slot_n(dev, n);
            std::unique_lock<std::mutex> l(w.mu, std::defer_lock);
            if (pass == 0) {
                if (!l.try_lock()) continue;
            } else {
                l.lock();
            }
            if (!group_usable(w, g, dev)) continue;
            lk = std::move(l);
            return &w;
        }
    return nullptr;
}

int g_cus[kMaxDev]; /* compute units per device (0: not read yet) */

/* the current device, or -1 (none, or past the tables here) */
int current_dev()
{
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxDev ? dev : -1;
}

bool ct_env()
{
    return switches().ct_ghash;
}

/* host-side phase times of the last request (ns, CLOCK_MONOTONIC): packed,
   doorbell written, done seen, returned — relative to the call's start */
thread_local uint64_t t_host[4];
inline uint64_t host_ns()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

/* A slot of device dev, locked (lk), its group running; ctx: the device
   address of h_ctx.  Nothing is posted yet when this fails. */
int claim_and_ensure(int dev, const void *h_ctx, std::unique_lock<std::mutex> &lk, Worker *&wp, uint64_t &ctx)
{
    wp = claim_worker(dev, lk);
    if (!wp) return NOISE_ERROR_NOT_APPLICABLE;
    Worker &w = *wp;
    t_last = wp;
    void *d_hctx = nullptr;
    if (h_ctx && hipHostGetDevicePointer(&d_hctx, (void *)h_ctx, 0) != hipSuccess)
        return NOISE_ERROR_NOT_APPLICABLE;
    ctx = (uint64_t)(uintptr_t)d_hctx;
    WorkerGroup &g = *w.g;
    {   /* the generation first, then launched / exiting (group_ensure) */
        const uint32_t gen0 = __atomic_load_n(&g.gen, __ATOMIC_ACQUIRE);
        const bool up = __atomic_load_n(&g.launched, __ATOMIC_ACQUIRE);
        if (!up || __atomic_load_n(&w.slot->exiting, __ATOMIC_ACQUIRE)) {
            const int rc = group_ensure(w, gen0, up ? 1 : 0);
            if (rc) return rc;
        }
    }
    /* after the launch (which starts the history afresh): this context may
       now sit in the workgroup's LDS cache */
    if (h_ctx) worker_note_ctx(w, h_ctx);
    if (debug_leave_before_post()) { /* test hook: the group leaves before k is posted */
        park_group(g);
        const uint64_t t0 = host_ns();
        while ((!__atomic_load_n(&w.slot->exiting, __ATOMIC_ACQUIRE) || hipStreamQuery(g.stream) != hipSuccess) &&
               host_ns() - t0 < 1000000000ull)
            __builtin_ia32_pause();
    }
    return NOISE_ERROR_NONE;
}

/* The next request of slot w: its stream, then its header (worker_proto.h).
   Returns its number; h1: the stream is packed. */
uint32_t post(Worker &w, const Request &rq, const uint8_t *key, const uint8_t *ad, const uint8_t *data, uint64_t &h1)
{
    const uint32_t k = ++w.seq;
    encode_stream(w.vram, (uint32_t *)w.in, w.tail, k, key, ad, rq.ad_len, data, rq.len + (rq.op ? 16u : 0u));
    h1 = host_ns();
    /* the data area before the header: sfence drains the write-combining
       buffers (device memory) and orders the stores (both) */
    _mm_sfence();
    __atomic_thread_fence(__ATOMIC_RELEASE);
    encode_header(w.vram, w.req, k, rq);
    _mm_sfence(); /* out of the write-combining buffer now, not later */
    return k;
}

/* Wait for the answer to request k, posted at h2.  A failure the worker
   caused (a relaunch that fails, no answer within WAIT_LIMIT_NS) is
   NOISE_ERROR_NOT_APPLICABLE: the caller runs the record through the launch
   path with the same nonce instead — the result is the same bytes, and the
   worker only ever writes w.out and the slot. */
int await(Worker &w, uint32_t k, const void *h_ctx, uint64_t h2)
{
    WorkerSlot *s = w.slot;
    WorkerGroup &g = *w.g;
    uint64_t spins = 0;
    while (__atomic_load_n(&s->done, __ATOMIC_ACQUIRE) != k) {
        __builtin_ia32_pause();
        if ((++spins & 1023) != 0) continue;
        const uint32_t gen0 = __atomic_load_n(&g.gen, __ATOMIC_ACQUIRE);
        if (__atomic_load_n(&s->exiting, __ATOMIC_ACQUIRE) && __atomic_load_n(&s->done, __ATOMIC_ACQUIRE) != k) {
            /* the group left before this slot took k: start it again (its
               workgroup starts at done = k - 1 and serves k) */
            const int rc = group_ensure(w, gen0, 2);
            if (rc) return rc;
            /* a relaunch by group_launch starts this slot's context history
               afresh, and the new workgroup serves k and caches h_ctx: note it
               again, or freeing the state would not park this group and the
               round keys would stay in its LDS */
            if (h_ctx) worker_note_ctx(w, h_ctx);
        }
        if (host_ns() - h2 > WAIT_LIMIT_NS) { /* no answer: drained, then reused */
            worker_abandon(w, k);
            return NOISE_ERROR_NOT_APPLICABLE;
        }
    }
    return NOISE_ERROR_NONE;
}

/* The answer to request k (st: what await returned) copied out, and the
   request scrubbed from the shared memory whatever became of it.  A stale
   input (status 2) is the worker's failure too: NOISE_ERROR_NOT_APPLICABLE. */
int collect_and_scrub(Worker &w, uint32_t k, const Request &rq, int st, uint8_t *data)
{
    if (st == NOISE_ERROR_NONE) {
        const uint32_t status = w.slot->status;
        st = status == 2 ? NOISE_ERROR_NOT_APPLICABLE : (status ? NOISE_ERROR_MAC_FAILURE : NOISE_ERROR_NONE);
        if (st == NOISE_ERROR_NONE) memcpy(data, w.out, rq.op ? rq.len : rq.len + 16);
    }
    scrub_request(w.vram, (uint32_t *)w.in, w.tail, w.out, k, rq.op, rq.len, rq.ad_len);
    return st;
}

/* the host view of slot `slot` of group `group` on the current device (debug hooks) */
const WorkerSlot *debug_slot(int group, int slot)
{
    const int dev = current_dev();
    if (dev < 0 || group < 0 || group >= kMaxGroups || slot < 0 || slot >= WORKER_MAX_SLOTS) return nullptr;
    return g_group[dev][group].slot[slot].slot;
}

} // namespace

extern "C" NA_HIDDEN int na_worker_enabled(void) { return worker_enabled() ? 1 : 0; }

/* A batch launch of `workgroups` workgroups on the current device: when it
   fills every CU, the resident workers of the device are asked to leave
   first.  A worker holds ~151 KB of its CU's LDS, so a batch workgroup
   placed on that CU could not start until it left (2 ms after its last
   request): the batch kernels are single generations per CU (C2: two
   one-lane workgroups per CU, C3: one AES-GCM workgroup), and one CU short
   would run a second generation on another CU. */
NA_HIDDEN void worker_park_for_batch(uint32_t workgroups)
{
    const int dev = current_dev();
    if (dev < 0) return;
    int cus = __atomic_load_n(&g_cus[dev], __ATOMIC_RELAXED);
    if (!cus) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            return;
        __atomic_store_n(&g_cus[dev], cus, __ATOMIC_RELAXED);
    }
    if (workgroups >= (uint32_t)cus && park_enabled()) park_device(dev);
}

/* A state's AES-GCM context (its pinned host copy h_ctx) is being freed:
   every worker that was sent it since its launch — and so may hold it in its
   LDS cache — leaves, scrubbing its LDS on the way out; the others stay. */
extern "C" NA_HIDDEN void na_worker_forget_ctx(const void *h_ctx)
{
    for (int d = 0; d < kMaxDev; ++d)
        for (int i = 0; i < kMaxGroups; ++i) {
            WorkerGroup &g = g_group[d][i];
            for (int k = 0; k < WORKER_MAX_SLOTS; ++k)
                if (worker_saw_ctx(g.slot[k], h_ctx)) {
                    park_group(g);
                    break;
                }
        }
}

/* One record through the resident worker: data holds len bytes (+ the tag
   for open) and receives CT || tag (seal) or, verified, the plaintext.  key:
   the raw ChaCha key; h_ctx / gen: AES-GCM, the pinned host copy of the
   state's context and the generation it was written at.  Returns
   NOISE_ERROR_NONE, _MAC_FAILURE, _SYSTEM, or _NOT_APPLICABLE (take the
   launch path). */
extern "C" NA_HIDDEN int na_worker_crypt(int cipher_id, const uint8_t *key, const void *h_ctx,
                                         uint32_t gen, uint64_t nonce, const uint8_t *ad,
                                         size_t ad_len, uint8_t *data, size_t len, int open)
{
    const uint64_t h0 = host_ns();
    if (cipher_id == NOISE_CIPHER_AESGCM && !h_ctx) return NOISE_ERROR_NOT_APPLICABLE;
    if (!worker_enabled() || len > WORKER_MAX_LEN || ad_len > WORKER_MAX_AD)
        return NOISE_ERROR_NOT_APPLICABLE;
    const int dev = current_dev();
    if (dev < 0) return NOISE_ERROR_NOT_APPLICABLE;
    std::unique_lock<std::mutex> lk;
    Worker *wp = nullptr;
    Request rq = {};
    const int rc = claim_and_ensure(dev, h_ctx, lk, wp, rq.ctx);
    if (rc) return rc;
    rq.op = open ? 1u : 0u;
    rq.ct = ct_env() ? 1u : 0u;
    rq.len = (uint32_t)len;
    rq.ad_len = (uint32_t)ad_len;
    rq.nonce = nonce;
    rq.cipher = (uint32_t)cipher_id;
    rq.gen = gen;
    uint64_t h1;
    const uint32_t k = post(*wp, rq, cipher_id == NOISE_CIPHER_CHACHAPOLY ? key : nullptr, ad, data, h1);
    const uint64_t h2 = host_ns();
    /* from here on every exit scrubs the shared memory */
    int st = await(*wp, k, h_ctx, h2);
    const uint64_t h3 = host_ns();
    st = collect_and_scrub(*wp, k, rq, st, data);
    const uint64_t h4 = host_ns();
    t_host[0] = h1 - h0; t_host[1] = h2 - h0; t_host[2] = h3 - h0; t_host[3] = h4 - h0;
    return st;
}

/* Test hook: the phase stamps of this thread's last worker request, in
   10-ns ticks relative to the moment the worker saw it: [0] fence done, [1]
   record and context in LDS, [2] computed, [3] results written, [4] release
   done; n = 5. */
extern "C" void noise_aead_debug_worker_stamps(uint32_t *out, int n)
{
    const WorkerSlot *s = t_last ? t_last->slot : nullptr;
    for (int i = 0; i < n && i < 5; ++i) out[i] = s ? s->stamps[i + 1] - s->stamps[0] : 0;
}

/* Test hook: this thread's last worker call on the host (ns from its
   start): request packed, doorbell written, done seen, returned. */
extern "C" void noise_aead_debug_worker_host_ns(uint64_t *out, int n)
{
    for (int i = 0; i < n && i < 4; ++i) out[i] = t_host[i];
}

/* Test hook: the latency-first path's s_memtime stamps (cycles from its
   start: ChaCha, CT in LDS, Poly blocks loaded, tree, tag, open's write). */
extern "C" void noise_aead_debug_worker_fast_stamps(uint32_t *out, int n)
{
    const WorkerSlot *s = t_last ? t_last->slot : nullptr;
    for (int i = 0; i < n && i < 8; ++i) out[i] = s ? s->fstamps[i] : 0;
}

/* Test hook: the placement of this thread's last worker: 0 none set up, 1
   requests in pinned host memory, 2 in device memory. */
extern "C" int noise_aead_debug_worker_placement(void)
{
    const Worker *w = t_last;
    return !w || w->state != 1 || !w->g || w->g->state != 1 ? 0 : (w->vram ? 2 : 1);
}

/* Test hook: request slots of the current device whose group is resident
   (each slot is one workgroup of its group's kernel). */
extern "C" int noise_aead_debug_workers_resident(void)
{
    const int dev = current_dev();
    if (dev < 0) return -1;
    int n = 0;
    for (int i = 0; i < kMaxGroups; ++i) {
        WorkerGroup &g = g_group[dev][i];
        std::lock_guard<std::mutex> lk(g.mu);
        if (g.state == 1 && g.launched && hipStreamQuery(g.stream) == hipErrorNotReady) n += g.nslots;
    }
    return n;
}

/* Test hook: worker kernels launched on the current device so far (a
   parked worker that is called again is relaunched). */
extern "C" unsigned noise_aead_debug_worker_launches(void)
{
    const int dev = current_dev();
    unsigned n = 0;
    for (int i = 0; dev >= 0 && i < kMaxGroups; ++i) n += __atomic_load_n(&g_group[dev][i].launches, __ATOMIC_RELAXED);
    return n;
}

/* Test hook: why slot `slot` of group `group` last left (stamps[7]: 1 stop,
   2 closing, 4 idle, 8 lifetime). */
extern "C" unsigned noise_aead_debug_worker_leave_reason(int group, int slot)
{
    const WorkerSlot *s = debug_slot(group, slot);
    return s ? s->stamps[7] : 0;
}

/* Test hook: that leave's born, now (10-ns ticks, low words), lifetime and
   launch number. */
extern "C" void noise_aead_debug_worker_leave_info(int group, int slot, unsigned *out)
{
    const WorkerSlot *s = debug_slot(group, slot);
    for (int i = 0; s && i < 4; ++i) out[i] = s->leave[i];
}

/* Test hook: per group of the current device, kernels launched (out[0..n)
   for groups 0..n-1), then the group_ensure counts by cause (debug). */
extern "C" void noise_aead_debug_worker_group_launches(unsigned *out, int n)
{
    const int dev = current_dev();
    if (dev < 0) return;
    for (int i = 0; i < n; ++i)
        out[i] = i < kMaxGroups ? __atomic_load_n(&g_group[dev][i].launches, __ATOMIC_RELAXED)
                                : (i - kMaxGroups < 4 ? g_dbg_ensure[i - kMaxGroups].load() : 0u);
}

/* Test hook: the shader clock (MHz) of the last worker request's compute
   phase (s_memtime cycles over s_memrealtime time). */
extern "C" double noise_aead_debug_worker_clock_mhz(void)
{
    const WorkerSlot *s = t_last ? t_last->slot : nullptr;
    if (!s || s->stamps[3] == s->stamps[2]) return 0.0;
    return (double)s->stamps[6] / ((double)(s->stamps[3] - s->stamps[2]) * 0.01);
}

} // namespace na
