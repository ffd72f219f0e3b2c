/*
 * transport.hip — device-resident transport sessions:
 * noise_aead_dev_transport_* (include/noise_aead_hip.h section 9).
 *
 * The object holds, for n sessions, a send and a receive key context and a
 * send and a receive nonce on the device, and what a call needs: descriptors
 * and statuses for max_frames records, per-session counts and bases, scan
 * scratch.  A call is handed every session's bytes in the echo wire format
 * and does per session what noise_wire_seal / _open / _echo do (wire.c), with
 * nothing coming back to the host:
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
 */
#include "launch.h"

#include "transport_plan.h"

#include <new>
#include <rocprim/device/device_scan.hpp>

using namespace na;

namespace {

#define TR_DEV __device__ __forceinline__

constexpr uint32_t TR_BLOCK = 64;
constexpr uint32_t TR_REFUSED_LEN = MAX_RECORD_LEN + 1; /* aead_kernels.h reject_len */

enum TrMode : uint32_t { TR_SEAL = 0, TR_OPEN = 1, TR_ECHO = 2 };

struct TrArgs {
    const uint8_t *wire;
    const uint64_t *off;
    const uint32_t *len;
    NoiseAeadTransportResult *result;
    uint64_t *send, *recv;       /* the nonces */
    uint64_t *count, *base;      /* per session: frames of the uncapped walk, their exclusive sum */
    uint32_t *frames, *consumed; /* per session, after the cap */
    int32_t *stop;
    RecDesc *recs, *seal_recs;   /* max_frames each; seal_recs: the echo's second job */
    const uint8_t *status;
    uint64_t ctx_bytes, max_frames;
    uint32_t n, mode;
};

TR_DEV uint64_t tr_start_nonce(const TrArgs &a, uint32_t i)
{
    if (a.mode == TR_SEAL) return a.send[i];
    if (a.mode == TR_OPEN) return a.recv[i];
    return a.send[i] > a.recv[i] ? a.send[i] : a.recv[i];
}

TR_DEV RecDesc tr_refused()
{
    RecDesc d = {};
    d.len = TR_REFUSED_LEN;
    return d;
}

__global__ __launch_bounds__(TR_BLOCK) void tr_count(TrArgs a)
{
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    a.count[i] = tr_walk(a.wire + a.off[i], a.len[i], tr_start_nonce(a, i), TR_NO_BUDGET).frames;
}

struct TrEmit {
    RecDesc *recs;
    uint64_t wire_off, nonce, ctx_off;
    TR_DEV void operator()(uint64_t k, uint64_t body, uint32_t L) const
    {
        RecDesc d;
        d.in_off = d.out_off = wire_off + body;
        d.nonce = nonce + k;
        d.ctx_off = ctx_off;
        d.ad_off = 0;
        d.len = L - TR_MAC_LEN;
        d.ad_len = 0;
        recs[k] = d;
    }
};

__global__ __launch_bounds__(TR_BLOCK) void tr_build(TrArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    const uint64_t all = a.base[a.n - 1] + a.count[a.n - 1];
    const uint64_t total = all < a.max_frames ? all : a.max_frames;
    if (t >= total && t < a.max_frames) a.recs[t] = tr_refused();
    if (t >= a.n) return;
    const uint32_t i = (uint32_t)t;
    bool cut;
    const uint64_t base = a.base[i], budget = tr_cap(base, a.count[i], a.max_frames, &cut);
    /* the session's context: send contexts first, then the receive ones */
    const bool seal = a.mode == TR_SEAL;
    const TrEmit emit = {a.recs + base, a.off[i], seal ? a.send[i] : a.recv[i],
                         (seal ? (uint64_t)i : (uint64_t)a.n + i) * a.ctx_bytes};
    TrWalk w = {0, 0, NOISE_ERROR_NONE};
    if (budget || !cut) w = tr_walk(a.wire + a.off[i], a.len[i], tr_start_nonce(a, i), budget, emit);
    if (cut) w.stop = NOISE_ERROR_NONE;
    if (seal) {
        a.send[i] += w.frames;
        const NoiseAeadTransportResult r = {(uint32_t)w.frames, (uint32_t)w.consumed, w.stop, 0};
        a.result[i] = r;
        return;
    }
    a.frames[i] = (uint32_t)w.frames;
    a.consumed[i] = (uint32_t)w.consumed;
    a.stop[i] = w.stop;
}

__global__ __launch_bounds__(TR_BLOCK) void tr_commit(TrArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
    const bool echo = a.mode == TR_ECHO;
    if (echo) {
        const uint64_t all = a.base[a.n - 1] + a.count[a.n - 1];
        const uint64_t total = all < a.max_frames ? all : a.max_frames;
        if (t >= total && t < a.max_frames) a.seal_recs[t] = tr_refused();
    }
    if (t >= a.n) return;
    const uint32_t i = (uint32_t)t;
    const uint32_t frames = a.frames[i];
    const uint64_t base = a.base[i]; /* base + frames <= max_frames (tr_cap); not read when frames == 0 */
    uint32_t prefix = 0;
    while (prefix < frames && a.status[base + prefix] == 0) ++prefix;
    NoiseAeadTransportResult r = {prefix, a.consumed[i], a.stop[i], 0};
    if (prefix < frames) { /* the first tag that failed wins over a later stop (wire.c wire_run) */
        r.consumed = (uint32_t)(a.recs[base + prefix].in_off - 2 - a.off[i]);
        r.error = NOISE_ERROR_MAC_FAILURE;
    }
    if (echo) {
        const uint64_t send = a.send[i];
        for (uint32_t k = 0; k < frames; ++k) {
            RecDesc d = tr_refused();
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
    a.result[i] = r;
}

size_t carve(size_t &off, size_t bytes)
{
    const size_t at = off;
    off += (bytes + 255) & ~(size_t)255;
    return at;
}

} // namespace

struct NoiseAeadDevTransport {
    int cipher_id, role;
    uint32_t n, max_frames;
    size_t ctx_bytes;
    /* one device allocation, carved */
    uint8_t *mem;
    size_t mem_bytes;
    uint8_t *ctx;             /* n send contexts, then n receive contexts */
    uint64_t *send, *recv, *count, *base;
    uint32_t *frames, *consumed;
    int32_t *stop;
    RecDesc *recs, *seal_recs;
    uint8_t *status;
    void *scan_tmp;
    size_t scan_bytes;
};

namespace {

typedef NoiseAeadDevTransport Tr;

int scan_counts(const Tr *tr, void *tmp, size_t &bytes, hipStream_t s)
{
    return hip_rc(rocprim::exclusive_scan(tmp, bytes, (const uint64_t *)tr->count, tr->base, (uint64_t)0, (size_t)tr->n,
                                          rocprim::plus<uint64_t>(), s));
}

int run(Tr *tr, TrMode mode, uint8_t *d_wire, const uint64_t *d_off, const uint32_t *d_len,
        NoiseAeadTransportResult *d_result, hipStream_t s)
{
    const int rc0 = tr_check_call(tr, tr ? tr->n : 0, d_wire, d_off, d_len, d_result);
    if (rc0 || !tr->n) return rc0;
    const TrArgs a = {d_wire, d_off, d_len, d_result, tr->send, tr->recv, tr->count, tr->base, tr->frames, tr->consumed,
                      tr->stop, tr->recs, tr->seal_recs, tr->status, tr->ctx_bytes, tr->max_frames, tr->n, mode};
    const uint32_t most = tr->n > tr->max_frames ? tr->n : tr->max_frames;
    const dim3 per_session((tr->n + TR_BLOCK - 1) / TR_BLOCK), padded((uint32_t)(((uint64_t)most + TR_BLOCK - 1) / TR_BLOCK));
    hipLaunchKernelGGL(tr_count, per_session, dim3(TR_BLOCK), 0, s, a);
    int rc = hip_rc(hipGetLastError());
    size_t bytes = tr->scan_bytes;
    if (!rc) rc = scan_counts(tr, tr->scan_tmp, bytes, s);
    if (rc) return rc;
    hipLaunchKernelGGL(tr_build, padded, dim3(TR_BLOCK), 0, s, a);
    rc = hip_rc(hipGetLastError());
    if (rc) return rc;
    NoiseAeadRagged job = {};
    job.ctx_base = tr->ctx;
    job.recs = (const NoiseAeadRecord *)tr->recs;
    job.in = job.out = d_wire;
    job.ad = d_wire; /* never read: every ad_len is 0 */
    job.status = tr->status;
    job.n_records = tr->max_frames;
    if (mode == TR_SEAL) return noise_aead_dev_seal_ragged(tr->cipher_id, &job, s);
    rc = noise_aead_dev_open_ragged(tr->cipher_id, &job, s);
    if (rc) return rc;
    hipLaunchKernelGGL(tr_commit, mode == TR_ECHO ? padded : per_session, dim3(TR_BLOCK), 0, s, a);
    rc = hip_rc(hipGetLastError());
    if (rc || mode == TR_OPEN) return rc;
    job.recs = (const NoiseAeadRecord *)tr->seal_recs;
    job.status = nullptr;
    return noise_aead_dev_seal_ragged(tr->cipher_id, &job, s);
}

} // namespace

extern "C" {

int noise_aead_dev_transport_new(NoiseAeadDevTransport **out, int cipher_id, int role, uint32_t n, const uint8_t *d_k1,
                                 const uint8_t *d_k2, uint32_t max_frames, void *stream)
{
    int rc = tr_check_new(out, cipher_id, role, n, d_k1, d_k2, max_frames);
    if (rc) return rc;
    *out = nullptr;
    Tr *tr = new (std::nothrow) Tr();
    if (!tr) return NOISE_ERROR_NO_MEMORY;
    tr->cipher_id = cipher_id;
    tr->role = role;
    tr->n = n;
    tr->max_frames = max_frames;
    tr->ctx_bytes = noise_aead_dev_ctx_bytes(cipher_id);
    if (n) {
        hipStream_t s = (hipStream_t)stream;
        rc = scan_counts(tr, nullptr, tr->scan_bytes, s); /* the size question: nothing is launched */
        if (rc) {
            delete tr;
            return rc;
        }
        const size_t ns = n, nf = max_frames;
        size_t off = 0;
        const size_t o_ctx = carve(off, 2 * ns * tr->ctx_bytes), o_send = carve(off, ns * 8), o_recv = carve(off, ns * 8);
        const size_t o_count = carve(off, ns * 8), o_base = carve(off, ns * 8), o_frames = carve(off, ns * 4);
        const size_t o_consumed = carve(off, ns * 4), o_stop = carve(off, ns * 4);
        const size_t o_recs = carve(off, nf * sizeof(RecDesc)), o_seal = carve(off, nf * sizeof(RecDesc));
        const size_t o_status = carve(off, nf), o_scan = carve(off, tr->scan_bytes);
        if (hipMalloc((void **)&tr->mem, off) != hipSuccess) {
            delete tr;
            return NOISE_ERROR_NO_MEMORY;
        }
        tr->mem_bytes = off;
        uint8_t *m = tr->mem;
        tr->ctx = m + o_ctx; tr->send = (uint64_t *)(m + o_send); tr->recv = (uint64_t *)(m + o_recv);
        tr->count = (uint64_t *)(m + o_count); tr->base = (uint64_t *)(m + o_base);
        tr->frames = (uint32_t *)(m + o_frames); tr->consumed = (uint32_t *)(m + o_consumed);
        tr->stop = (int32_t *)(m + o_stop); tr->recs = (RecDesc *)(m + o_recs); tr->seal_recs = (RecDesc *)(m + o_seal);
        tr->status = m + o_status; tr->scan_tmp = m + o_scan;
        /* every nonce starts at 0; the initiator sends under k1, the responder under k2 */
        const bool init = role == NOISE_ROLE_INITIATOR;
        rc = hip_rc(hipMemsetAsync(tr->mem, 0, tr->mem_bytes, s));
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

int noise_aead_dev_transport_free(NoiseAeadDevTransport *tr)
{
    if (!tr) return NOISE_ERROR_INVALID_PARAM;
    int rc = NOISE_ERROR_NONE;
    if (tr->mem) {
        /* work of this object may still be in flight on the caller's streams */
        rc = hip_rc(hipDeviceSynchronize());
        const int rc2 = hip_rc(hipMemset(tr->mem, 0, tr->mem_bytes));
        const int rc3 = hip_rc(hipFree(tr->mem));
        rc = rc ? rc : (rc2 ? rc2 : rc3);
    }
    memset((void *)tr, 0, sizeof(*tr));
    delete tr;
    return rc;
}

uint64_t *noise_aead_dev_transport_nonces(const NoiseAeadDevTransport *tr, int direction)
{
    if (!tr || (direction != 0 && direction != 1)) return nullptr;
    return direction ? tr->recv : tr->send;
}

int noise_aead_dev_transport_seal_frames(NoiseAeadDevTransport *tr, uint8_t *d_wire, const uint64_t *d_off,
                                         const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream)
{
    return run(tr, TR_SEAL, d_wire, d_off, d_len, d_result, (hipStream_t)stream);
}

int noise_aead_dev_transport_open_frames(NoiseAeadDevTransport *tr, uint8_t *d_wire, const uint64_t *d_off,
                                         const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream)
{
    return run(tr, TR_OPEN, d_wire, d_off, d_len, d_result, (hipStream_t)stream);
}

int noise_aead_dev_transport_echo_frames(NoiseAeadDevTransport *tr, uint8_t *d_wire, const uint64_t *d_off,
                                         const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream)
{
    return run(tr, TR_ECHO, d_wire, d_off, d_len, d_result, (hipStream_t)stream);
}

} // extern "C"
