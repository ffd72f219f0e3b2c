/*
 * kdf.hip — session key fan-out on the GPU.
 *
 * A server that completes many handshakes holds one chaining key ck per
 * session; noise_symmetricstate_split (symmetricstate.c:514-573) turns each
 * into the two transport keys with HKDF(ck, "") (hashstate.c:476-516) and
 * noise_symmetricstate_mix_key does HKDF(ck, ikm) during the handshake.
 * hkdf_batch runs that for a whole batch of sessions, one lane per session,
 * for the four Noise hashes (constants.h:43-46):
 *   SHA-256 / SHA-512 (FIPS 180-4; src/crypto/sha2), BLAKE2s / BLAKE2b
 *   (RFC 7693, unkeyed; src/crypto/blake2), HMAC as noise_hashstate_hmac
 *   (hashstate.c:407-448: the key hashed when longer than a block,
 *   zero-padded, ipad 0x36 / opad 0x5c).
 * Its outputs are the raw keys noise_aead_dev_prepare turns into key
 * contexts, so a batch of finished handshakes becomes a batch of transport
 * CipherStates without leaving the device.
 *
 * The arithmetic itself — HMAC, HKDF, MixHash — is hasher.h's, shared with
 * the batched handshakes (handshake.hip); the kernels here are the batch
 * loads and stores around it.
 *
 * This is scalar per-lane work (a split is 6 compressions), not a hot loop;
 * it is written for clarity and checked byte for byte against the oracle
 * and the reference's own HKDF outputs (tests/golden/hkdf.json).
 */
#pragma once
#include "aead_device.h"
#include "hasher.h"

namespace na {

/* workgroup sizes: one lane per session or record; commit_hash, one per byte of h */
constexpr uint32_t KDF_BLOCK = 64, KDF_COMMIT_BLOCK = 256;

struct KdfArgs {
    int hash_id;
    const uint8_t *keys;
    const uint8_t *data;
    uint8_t *out1, *out2;
    uint32_t hlen, key_len, data_len, out1_len, out2_len, n;
};

/* kdf_hkdf (hasher.h), one lane per session; the outputs are stored truncated
   to out1_len and out2_len (hashstate.c:496-497 allows up to the hash's length) */
__global__ __launch_bounds__(KDF_BLOCK) void hkdf_batch(KdfArgs a)
{
    const uint32_t i = blockIdx.x * KDF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const uint8_t *key = a.keys + (size_t)i * a.key_len;
    const uint8_t *data = a.data ? a.data + (size_t)i * a.data_len : nullptr;
    uint8_t o1[64], o2[64];
    kdf_hkdf(a.hash_id, a.hlen, key, a.key_len, data, a.data_len, o1, o2);
    for (uint32_t j = 0; j < a.out1_len; ++j) a.out1[(size_t)i * a.out1_len + j] = o1[j];
    for (uint32_t j = 0; j < a.out2_len; ++j) a.out2[(size_t)i * a.out2_len + j] = o2[j];
}

/* ------------------------------------------------ handshake-payload MixHash
 *
 * noise_symmetricstate_{encrypt,decrypt}_and_hash (symmetricstate.c
 * :352-445) for a batch of SymmetricStates: after (before, for decrypt) the
 * AEAD of record i under AD = h_i, h_i = HASH(h_i || ciphertext_i || tag_i)
 * (noise_symmetricstate_mix_hash, :244-258).  One lane per record. */
struct MixHashArgs {
    int hash_id;
    uint32_t hlen, n;
    const uint8_t *h_in;
    uint8_t *h_out;
    const uint8_t *base;   /* the job's `out` (encrypt) or `in` (decrypt) */
    const RecDesc *recs;
    int use_out_off;
};

__global__ __launch_bounds__(KDF_BLOCK) void mix_hash_batch(MixHashArgs a)
{
    const uint32_t i = blockIdx.x * KDF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const RecDesc d = a.recs[i];
    uint8_t h[64];
    load_row(h, a.h_in, i, a.hlen);
    kdf_mix_hash(a.hash_id, a.hlen, h, a.base + (a.use_out_off ? d.out_off : d.in_off), d.len + 16);
    store_row(a.h_out, i, a.hlen, h);
}

/* decrypt_and_hash keeps the new hash only when the tag verified (:436-443) */
__global__ __launch_bounds__(KDF_COMMIT_BLOCK) void commit_hash(uint8_t *h, const uint8_t *h_new,
                                                                const uint8_t *status, uint32_t hlen, uint32_t n)
{
    const uint64_t t = (uint64_t)blockIdx.x * KDF_COMMIT_BLOCK + threadIdx.x;
    if (t >= (uint64_t)n * hlen) return;
    if (status[t / hlen] == 0) h[t] = h_new[t];
}

} // namespace na
