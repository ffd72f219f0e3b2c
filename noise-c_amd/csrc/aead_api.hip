/*
 * aead_api.hip — the thin C-ABI layer between the plain-C host front end
 * (cipherstate.c) and the gfx950 kernels.  Device-resident entry points of
 * include/noise_aead_hip.h: plain pointers, sizes and an opaque stream; no
 * C++ or torch types cross this boundary.  HIP errors map to
 * NOISE_ERROR_SYSTEM (constants.h:137), bad arguments to
 * NOISE_ERROR_INVALID_PARAM / _INVALID_LENGTH / _UNKNOWN_ID.
 */
#include "launch.h"

#include "kdf.hip"
#include "pad.hip"

using namespace na;

namespace {

UniformArgs to_args(const NoiseAeadUniform *j, uint32_t balance, uint32_t vf)
{
    UniformArgs a;
    a.keys = (const uint8_t *)j->ctx;
    a.nonce_base = j->nonce_base;
    a.in = j->in;
    a.out = j->out;
    a.ad = j->ad;
    a.status = j->status;
    a.in_stride = j->in_stride;
    a.out_stride = j->out_stride;
    a.ad_stride = j->ad_stride;
    a.rps = j->recs_per_state;
    a.n_records = j->n_records;
    a.len = j->len;
    a.ad_len = j->ad_len;
    a.balance = balance;
    a.vf = vf;
    return a;
}

/* what the ChaChaPoly plans ask of the device */
uint32_t cus_for(int cipher_id) { return cipher_id == NOISE_CIPHER_CHACHAPOLY ? device_cus() : 0; }

/* the calling thread's last launched plan (noise_aead_debug_last_plan) */
thread_local Plan t_last_plan;

/* Every entry point: check the job, plan it (dispatch.h), launch the plan. */
int launch_plan(const Plan &p, const PlanArgs &args, void *stream)
{
    if (p.rc) return p.rc;
    if (p.grid) t_last_plan = p;
    if (!plan_is_gcm(p)) return chacha_launch(p, args, (hipStream_t)stream);
    const int rc = hip_rc(ensure_aes_tables());
    return rc ? rc : aes_launch(p, args, (hipStream_t)stream);
}

int run_uniform(int cipher_id, const NoiseAeadUniform *job, void *stream, bool open)
{
    const int rc = check_uniform(job, open);
    if (rc) return rc;
    const Plan p = plan_uniform(cipher_id, job, open, switches(), cus_for(cipher_id));
    const UniformArgs a = to_args(job, p.balance, p.vf);
    return launch_plan(p, {&a, nullptr, nullptr}, stream);
}

int run_duplex(int cipher_id, const NoiseAeadUniform *sj, const NoiseAeadUniform *oj, void *stream)
{
    int rc = check_duplex(sj, oj);
    if (rc) return rc;
    const Plan p = plan_duplex(cipher_id, sj, oj, switches(), cus_for(cipher_id));
    if (p.shared) {
        const UniformArgs sa = to_args(sj, p.balance, 0), oa = to_args(oj, p.balance, p.vf);
        return launch_plan(p, {&sa, &oa, nullptr}, stream);
    }
    rc = run_uniform(cipher_id, sj, stream, false);
    if (!rc) rc = run_uniform(cipher_id, oj, stream, true);
    return rc;
}

RaggedArgs to_args(const NoiseAeadRagged *job, uint32_t vf)
{
    RaggedArgs a;
    a.keys = (const uint8_t *)job->ctx_base;
    a.recs = (const RecDesc *)job->recs;
    a.in = job->in;
    a.out = job->out;
    a.ad = job->ad;
    a.status = job->status;
    a.n_records = job->n_records;
    a.vf = vf;
    return a;
}

int run_ragged(int cipher_id, const NoiseAeadRagged *job, void *stream, bool open)
{
    const int rc = check_ragged(job);
    if (rc) return rc;
    const uint32_t resident = ragged_takes_seg(cipher_id, job, switches()) ? seg_resident(open ? SEG_OPEN : SEG_SEAL) : 0;
    const Plan p = plan_ragged(cipher_id, job, open, switches(), resident);
    const RaggedArgs a = to_args(job, p.vf);
    return launch_plan(p, {nullptr, nullptr, &a, nullptr}, stream);
}

int run_duplex_ragged(int cipher_id, const NoiseAeadRagged *sj, const NoiseAeadRagged *oj, void *stream)
{
    int rc = check_duplex_ragged(sj, oj);
    if (rc) return rc;
    /* the occupancy of the kernel the segmented jobs would take */
    const bool seg_s = ragged_takes_seg(cipher_id, sj, switches()), seg_o = ragged_takes_seg(cipher_id, oj, switches());
    const uint32_t resident =
        seg_s && seg_o ? seg_resident(SEG_DUPLEX) : (seg_s ? seg_resident(SEG_SEAL) : (seg_o ? seg_resident(SEG_OPEN) : 0));
    const Plan p = plan_duplex_ragged(cipher_id, sj, oj, switches(), resident);
    if (p.rc) return p.rc;
    if (p.shared) {
        const RaggedArgs sa = to_args(sj, 0), oa = to_args(oj, p.vf);
        return launch_plan(p, {nullptr, nullptr, &sa, &oa}, stream);
    }
    rc = run_ragged(cipher_id, sj, stream, false);
    if (!rc) rc = run_ragged(cipher_id, oj, stream, true);
    return rc;
}

__global__ void splitmix_fill(uint8_t *out, uint64_t nbytes, uint64_t seed, uint64_t word0)
{
    const uint64_t nw = nbytes / 8;
    for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w * 8 < nbytes;
         w += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t z = seed + word0 + w + 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        if (w < nw) {
            ((uint64_t *)out)[w] = z;
        } else {
            for (uint64_t b = 0; b < nbytes - 8 * w; ++b) out[8 * w + b] = (uint8_t)(z >> (8 * b));
        }
    }
}

} // namespace

static_assert(sizeof(NoiseAeadRecord) == sizeof(RecDesc), "record descriptor layout");
static_assert(sizeof(NoiseRandSnapshot) == sizeof(RandSnap), "RandState snapshot layout");
static_assert(offsetof(NoiseAeadRecord, ctx_off) == offsetof(RecDesc, ctx_off), "layout");

extern "C" {

size_t noise_aead_dev_ctx_bytes(int cipher_id)
{
    if (cipher_id == NOISE_CIPHER_CHACHAPOLY) return 32;
    if (cipher_id == NOISE_CIPHER_AESGCM) return sizeof(AesCtx);
    return 0;
}

int noise_aead_dev_prepare(int cipher_id, const uint8_t *d_raw_keys, uint32_t n_states,
                           void *d_ctx, void *stream)
{
    if (!d_raw_keys || !d_ctx) return NOISE_ERROR_INVALID_PARAM;
    if (n_states == 0) return NOISE_ERROR_NONE;
    hipStream_t s = (hipStream_t)stream;
    if (cipher_id == NOISE_CIPHER_CHACHAPOLY)
        return hip_rc(hipMemcpyAsync(d_ctx, d_raw_keys, (size_t)n_states * 32,
                                     hipMemcpyDeviceToDevice, s));
    if (cipher_id == NOISE_CIPHER_AESGCM) {
        int rc = hip_rc(ensure_aes_tables());
        if (rc) return rc;
        return aes_prepare(d_raw_keys, n_states, d_ctx, s);
    }
    return NOISE_ERROR_UNKNOWN_ID;
}

int noise_aead_dev_seal_uniform(int cipher_id, const NoiseAeadUniform *job, void *stream)
{
    return run_uniform(cipher_id, job, stream, false);
}

int noise_aead_dev_open_uniform(int cipher_id, const NoiseAeadUniform *job, void *stream)
{
    return run_uniform(cipher_id, job, stream, true);
}

int noise_aead_dev_duplex_uniform(int cipher_id, const NoiseAeadUniform *seal_job,
                                  const NoiseAeadUniform *open_job, void *stream)
{
    return run_duplex(cipher_id, seal_job, open_job, stream);
}

int noise_aead_dev_seal_ragged(int cipher_id, const NoiseAeadRagged *job, void *stream)
{
    return run_ragged(cipher_id, job, stream, false);
}

int noise_aead_dev_open_ragged(int cipher_id, const NoiseAeadRagged *job, void *stream)
{
    return run_ragged(cipher_id, job, stream, true);
}

int noise_aead_dev_duplex_ragged(int cipher_id, const NoiseAeadRagged *seal_job,
                                 const NoiseAeadRagged *open_job, void *stream)
{
    return run_duplex_ragged(cipher_id, seal_job, open_job, stream);
}

int noise_aead_dev_fill_splitmix(uint8_t *d_out, uint64_t nbytes, uint64_t seed,
                                 uint64_t word0, void *stream)
{
    if (!d_out) return NOISE_ERROR_INVALID_PARAM;
    if (!nbytes) return NOISE_ERROR_NONE;
    uint64_t words = (nbytes + 7) / 8;
    uint32_t blocks = (uint32_t)((words + 255) / 256);
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(splitmix_fill, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_out,
                       nbytes, seed, word0);
    return hip_rc(hipGetLastError());
}

int noise_aead_dev_hkdf(int hash_id, const uint8_t *d_keys, uint32_t key_len,
                        const uint8_t *d_data, uint32_t data_len, uint32_t n, uint8_t *d_out1,
                        uint32_t out1_len, uint8_t *d_out2, uint32_t out2_len, void *stream)
{
    const uint32_t hl = hash_len(hash_id);
    if (!hl) return NOISE_ERROR_UNKNOWN_ID;
    if (!n) return NOISE_ERROR_NONE;
    if (!d_keys || !d_out1 || !d_out2 || (data_len && !d_data)) return NOISE_ERROR_INVALID_PARAM;
    /* hashstate.c:496-497 */
    if (out1_len > hl || out2_len > hl) return NOISE_ERROR_INVALID_LENGTH;
    if (key_len == 0 || key_len > KDF_MAX_IN || data_len > KDF_MAX_IN)
        return NOISE_ERROR_INVALID_LENGTH;
    KdfArgs a;
    a.hash_id = hash_id;
    a.keys = d_keys;
    a.data = data_len ? d_data : nullptr;
    a.out1 = d_out1;
    a.out2 = d_out2;
    a.hlen = hl;
    a.key_len = key_len;
    a.data_len = data_len;
    a.out1_len = out1_len;
    a.out2_len = out2_len;
    a.n = n;
    return launch_items(hkdf_batch, n, KDF_BLOCK, (hipStream_t)stream, a);
}

int noise_aead_dev_split(int hash_id, const uint8_t *d_ck, uint32_t n, uint8_t *d_k1,
                         uint8_t *d_k2, void *stream)
{
    /* an unknown id: key_len 0 here, and noise_aead_dev_hkdf answers UNKNOWN_ID before it looks at it */
    return noise_aead_dev_hkdf(hash_id, d_ck, hash_len(hash_id), nullptr, 0, n, d_k1, 32, d_k2, 32, stream);
}

static int launch_mix_hash(int hash_id, uint32_t hl, const uint8_t *h_in, uint8_t *h_out,
                           const NoiseAeadRagged *job, bool use_out, hipStream_t s)
{
    MixHashArgs m;
    m.hash_id = hash_id;
    m.hlen = hl;
    m.n = job->n_records;
    m.h_in = h_in;
    m.h_out = h_out;
    m.base = use_out ? job->out : job->in;
    m.recs = (const RecDesc *)job->recs;
    m.use_out_off = use_out;
    return launch_items(mix_hash_batch, job->n_records, KDF_BLOCK, s, m);
}

int noise_aead_dev_encrypt_and_hash(int cipher_id, int hash_id, uint8_t *d_h,
                                    const NoiseAeadRagged *job, void *stream)
{
    const uint32_t hl = hash_len(hash_id);
    if (!hl) return NOISE_ERROR_UNKNOWN_ID;
    if (!d_h || !job || job->ad != d_h) return NOISE_ERROR_INVALID_PARAM;
    if (job->n_records == 0) return NOISE_ERROR_NONE;
    int rc = run_ragged(cipher_id, job, stream, false);
    if (rc) return rc;
    return launch_mix_hash(hash_id, hl, d_h, d_h, job, true, (hipStream_t)stream);
}

int noise_aead_dev_decrypt_and_hash(int cipher_id, int hash_id, uint8_t *d_h,
                                    const NoiseAeadRagged *job, void *stream)
{
    const uint32_t hl = hash_len(hash_id);
    if (!hl) return NOISE_ERROR_UNKNOWN_ID;
    if (!d_h || !job || job->ad != d_h || !job->status) return NOISE_ERROR_INVALID_PARAM;
    if (job->n_records == 0) return NOISE_ERROR_NONE;
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)job->n_records * hl;
    uint8_t *h_new = nullptr;
    /* stream-ordered pool allocation: no device synchronisation, and after
       the first call the pool hands the same memory back */
    if (hipMallocAsync((void **)&h_new, bytes, s) != hipSuccess) return NOISE_ERROR_NO_MEMORY;
    /* hash the ciphertext before the (in-place) decryption overwrites it */
    int rc = launch_mix_hash(hash_id, hl, d_h, h_new, job, false, s);
    if (!rc) rc = run_ragged(cipher_id, job, stream, true);
    if (!rc) /* one lane per byte of h */
        rc = launch_items(commit_hash, (uint64_t)job->n_records * hl, KDF_COMMIT_BLOCK, s, d_h, h_new, job->status, hl,
                          job->n_records);
    (void)hipFreeAsync(h_new, s);
    return rc;
}

int noise_aead_dev_pad(NoiseRandSnapshot *d_rand, uint8_t *d_payloads, uint64_t stride,
                       const uint32_t *d_orig_lens, uint32_t padded_len, uint32_t n,
                       int padding_mode, uint32_t *d_done, void *stream)
{
    if (!d_payloads || (n && !d_orig_lens)) return NOISE_ERROR_INVALID_PARAM;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) { /* NULL state: INVALID_PARAM on both branches (randstate.c:356-362) */
        const int rc = d_done ? hip_rc(hipMemsetAsync(d_done, 0, sizeof(uint32_t), s)) : NOISE_ERROR_NONE;
        return rc ? rc : (d_rand ? NOISE_ERROR_NONE : NOISE_ERROR_INVALID_PARAM);
    }
    if (!d_rand || padding_mode == NOISE_PADDING_ZERO) {
        /* randstate.c:356-362: without a state the padding is zeroed anyway */
        hipLaunchKernelGGL(pad_zero, dim3(n < 65535u ? n : 65535u), dim3(256), 0, s, d_payloads,
                           stride, d_orig_lens, padded_len, n, d_done);
        const int rc = hip_rc(hipGetLastError());
        return rc ? rc : (d_rand ? NOISE_ERROR_NONE : NOISE_ERROR_INVALID_PARAM);
    }
    hipLaunchKernelGGL(pad_random, dim3(1), dim3(64), 0, s, (RandSnap *)d_rand, d_payloads, stride,
                       d_orig_lens, padded_len, n, d_done);
    return hip_rc(hipGetLastError());
}

/* The lane questions: each answered by the plans' own lane rule (FAST
   layouts, automatic lanes). */
int noise_aead_dev_default_lanes(int cipher_id, uint32_t n_records)
{
    if (cipher_id == NOISE_CIPHER_CHACHAPOLY) return chacha_uniform_lanes(0, n_records, true, false, switches());
    return cipher_id == NOISE_CIPHER_AESGCM ? (int)PLAN_GCM_LANES : 0;
}

int noise_aead_dev_duplex_lanes(int cipher_id, uint32_t n_records)
{
    if (cipher_id == NOISE_CIPHER_CHACHAPOLY) return chacha_uniform_lanes(0, n_records, true, true, switches());
    return noise_aead_dev_default_lanes(cipher_id, n_records);
}

/* host_internal.h: the host paths know their records' lengths */
NA_HIDDEN uint32_t na_chacha_lanes(uint32_t n_records, uint32_t max_len)
{
    return host_chacha_lanes(n_records, max_len, switches());
}

NA_HIDDEN uint32_t na_aes_lanes(uint32_t n_records)
{
    (void)n_records;
    return host_aes_lanes(switches());
}

int noise_aead_debug_last_plan(char *buf, size_t n)
{
    return plan_print(t_last_plan, buf, n);
}

} // extern "C"
