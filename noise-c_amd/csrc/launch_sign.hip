/*
 * launch_sign.hip — batched Ed25519: noise_aead_dev_sign_verify,
 * noise_aead_dev_sign_public and noise_aead_dev_sign (include/noise_aead_hip.h
 * section 17).  A translation unit of its own, as launch_dh.hip is, so the
 * build stays parallel and the resource check of tests/test_sign_host.py
 * compiles it alone.
 *
 * One lane per entry, 64-lane workgroups.  A lane first hashes (SHA-512
 * through hasher.h's Hasher, whose byte buffer is the only memory a lane
 * indexes by data), reduces the digest mod L in registers (sc25519.h) and then
 * walks the curve (ge25519.h, on fe25519.h's eight 32-bit limbs).  The hash
 * phases are functions of their own that are not inlined, so that the
 * Hasher's buffers are dead before the walk starts and the walk keeps its
 * points in registers.  The host checks (dispatch.h check_sign_*) run before
 * any launch.
 */
#include "launch.h"

#include "hasher.h"
#include "ge25519.h"

using namespace na;

namespace {

constexpr uint32_t SIGN_BLOCK = 64;
constexpr uint8_t STATUS_SIGNATURE_REFUSED = 6;

struct VerifyArgs {
    const uint8_t *pub, *sig, *msg;
    const uint64_t *msg_off;
    const uint32_t *msg_len;
    const uint8_t *status_in;
    uint8_t *status;
    uint64_t pub_stride, sig_stride;
    uint32_t n;
};

struct SignArgs {
    const uint8_t *priv, *pub, *msg;
    const uint64_t *msg_off;
    const uint32_t *msg_len;
    uint8_t *out;
    uint64_t priv_stride, pub_stride;
    uint32_t n;
};

/* What the hash phases hand the walks, by value: registers, not memory. */
struct Seed { Sc a; F25 prefix; };

__device__ __forceinline__ Sc finish_mod_l(Hasher &H)
{
    uint8_t digest[64];
    H.final(digest);
    const Sc r = sc_from_bytes64(digest);
    for (int i = 0; i < 64; ++i) digest[i] = 0;
    return r;
}

/* h = SHA-512(R || A || M) mod L (ed25519_hram): all three in device memory */
__device__ __noinline__ Sc hash_ram(const uint8_t *r, const uint8_t *pub, const uint8_t *m, uint32_t nm)
{
    Hasher H;
    H.init(H_SHA512);
    H.update(r, 32);
    H.update(pub, 32);
    H.update(m, nm);
    return finish_mod_l(H);
}

/* r = SHA-512(prefix || M) mod L: the prefix goes straight into the Hasher's
   block buffer, the one place a lane's secret bytes are indexed */
__device__ __noinline__ Sc hash_r(F25 prefix, const uint8_t *m, uint32_t nm)
{
    Hasher H;
    H.init(H_SHA512);
    f25_store(H.buf, prefix);
    H.fill = 32;
    H.total = 32;
    H.update(m, nm);
    return finish_mod_l(H);
}

/* ed25519_extsk of a seed: the clamped scalar mod L, and the 32-byte prefix
   the r hash starts with */
__device__ __noinline__ Seed expand_seed(const uint8_t *seed)
{
    Hasher H;
    uint8_t digest[64];
    H.init(H_SHA512);
    H.update(seed, 32);
    H.final(digest);
    digest[0] &= 248;
    digest[31] &= 127;
    digest[31] |= 64;
    Seed s;
    s.a = sc_from_bytes32(digest);
    s.prefix = f25_load(digest + 32);
    for (int i = 0; i < 64; ++i) digest[i] = 0;
    return s;
}

/* Entry i is ed25519_sign_open (ed25519.c:93-116).  Everything it reads is
   public, so the refusals leave early. */
__global__ void __launch_bounds__(SIGN_BLOCK) ed25519_verify_batch(VerifyArgs a)
{
    const uint32_t i = blockIdx.x * SIGN_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    if (a.status_in) {
        /* a failed entry does no work and reads nothing of its own */
        const uint8_t st = a.status_in[i];
        if (st) {
            a.status[i] = st;
            return;
        }
    }
    const uint8_t *pub = a.pub + (uint64_t)i * a.pub_stride;
    const uint8_t *sig = a.sig + (uint64_t)i * a.sig_stride;
    Ge na_;
    if ((sig[63] & 0xE0) || !ge_decode_negative(na_, pub)) {
        a.status[i] = STATUS_SIGNATURE_REFUSED;
        return;
    }
    const Sc h = hash_ram(sig, pub, a.msg + a.msg_off[i], a.msg_len[i]);
    const Sc s = sc_from_bytes32(sig + 32);
    const F25 check = ge_encode(ge_double_scalarmult(s, h, na_));
    const F25 r = f25_load(sig);
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) diff |= check.v[j] ^ r.v[j];
    a.status[i] = diff ? STATUS_SIGNATURE_REFUSED : 0;
}

/* ed25519_publickey (ed25519.c:45-55) of each seed */
__global__ void __launch_bounds__(SIGN_BLOCK) ed25519_public_batch(SignArgs a)
{
    const uint32_t i = blockIdx.x * SIGN_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const Seed s = expand_seed(a.priv + (uint64_t)i * a.priv_stride);
    f25_store(a.out + (uint64_t)i * 32, ge_encode(ge_scalarmult_base(s.a)));
}

/* ed25519_sign (ed25519.c:58-91): the public key is taken as given */
__global__ void __launch_bounds__(SIGN_BLOCK) ed25519_sign_batch(SignArgs a)
{
    const uint32_t i = blockIdx.x * SIGN_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const uint8_t *msg = a.msg + a.msg_off[i];
    const uint32_t len = a.msg_len[i];
    uint8_t *out = a.out + (uint64_t)i * 64;
    const Seed s = expand_seed(a.priv + (uint64_t)i * a.priv_stride);
    const Sc r = hash_r(s.prefix, msg, len);
    /* R goes to the output first: the second hash reads it from there */
    f25_store(out, ge_encode(ge_scalarmult_base(r)));
    const Sc h = hash_ram(out, a.pub + (uint64_t)i * a.pub_stride, msg, len);
    sc_store(out + 32, sc_muladd(h, s.a, r));
}

} // namespace

extern "C" {

int noise_aead_dev_sign_verify(int sign_id, const uint8_t *d_pub, uint64_t pub_stride, const uint8_t *d_sig,
                               uint64_t sig_stride, const uint8_t *d_msg, const uint64_t *d_msg_off,
                               const uint32_t *d_msg_len, uint32_t n, const uint8_t *d_status_in, uint8_t *d_status,
                               void *stream)
{
    const int rc = check_sign_verify(sign_id, d_pub, pub_stride, d_sig, sig_stride, d_msg, d_msg_off, d_msg_len, n,
                                     d_status_in, d_status);
    if (rc || !n) return rc;
    const VerifyArgs a = {d_pub, d_sig, d_msg, d_msg_off, d_msg_len, d_status_in, d_status, pub_stride, sig_stride, n};
    return launch_items(ed25519_verify_batch, n, SIGN_BLOCK, (hipStream_t)stream, a);
}

int noise_aead_dev_sign_public(int sign_id, const uint8_t *d_priv, uint64_t priv_stride, uint32_t n,
                               uint8_t *d_pub_out, void *stream)
{
    const int rc = check_sign_public(sign_id, d_priv, priv_stride, n, d_pub_out);
    if (rc || !n) return rc;
    const SignArgs a = {d_priv, nullptr, nullptr, nullptr, nullptr, d_pub_out, priv_stride, 0, n};
    return launch_items(ed25519_public_batch, n, SIGN_BLOCK, (hipStream_t)stream, a);
}

int noise_aead_dev_sign(int sign_id, const uint8_t *d_priv, uint64_t priv_stride, const uint8_t *d_pub,
                        uint64_t pub_stride, const uint8_t *d_msg, const uint64_t *d_msg_off,
                        const uint32_t *d_msg_len, uint32_t n, uint8_t *d_sig_out, void *stream)
{
    const int rc = check_sign(sign_id, d_priv, priv_stride, d_pub, pub_stride, d_msg, d_msg_off, d_msg_len, n,
                              d_sig_out);
    if (rc || !n) return rc;
    const SignArgs a = {d_priv, d_pub, d_msg, d_msg_off, d_msg_len, d_sig_out, priv_stride, pub_stride, n};
    return launch_items(ed25519_sign_batch, n, SIGN_BLOCK, (hipStream_t)stream, a);
}

} // extern "C"
