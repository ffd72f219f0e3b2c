/*
 * noise_aead_hip.h — C ABI of the MI355X (gfx950) transport AEAD engine.
 *
 * Drop-in for noise-c's CipherState path (rweather/noise-c v0.0.1):
 *
 *  1. The reference's public CipherState API, same names, signatures,
 *     validation and error codes (include/noise/protocol/cipherstate.h:34-53,
 *     src/protocol/cipherstate.c:77-555).  Link this library in place of the
 *     CipherState part of libnoiseprotocol.
 *  2. The reference's cipher plugin constructors (src/protocol/internal.h:
 *     655-656) returning objects whose first member has the exact layout of
 *     struct NoiseCipherState_s (internal.h:58-146), so the reference's own
 *     cipherstate.c / symmetricstate.c keep working against them.
 *  3. Additive batch entry points (host buffers): N records, any mix of
 *     CipherStates, one GPU pass — results identical to N sequential calls.
 *  4. Device-resident entry points: records, keys and nonces already in HBM.
 *
 * Every computation on the encrypt/decrypt path runs in the gfx950 kernels;
 * there is no CPU fallback.  Without a usable GPU the crypto entry points
 * return NOISE_ERROR_SYSTEM.
 */
#ifndef NOISE_AEAD_HIP_H
#define NOISE_AEAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------- reference types/constants */

#ifndef NOISE_BUFFER_H
#define NOISE_BUFFER_H
/* include/noise/protocol/buffer.h:33-48 */
typedef struct {
    uint8_t *data;
    size_t size;
    size_t max_size;
} NoiseBuffer;
#define noise_buffer_init(buffer) \
    ((buffer).data = 0, (buffer).size = 0, (buffer).max_size = 0)
#define noise_buffer_set_output(buffer, ptr, len) \
    ((buffer).data = (ptr), (buffer).size = 0, (buffer).max_size = (len))
#define noise_buffer_set_input(buffer, ptr, len) \
    ((buffer).data = (ptr), (buffer).size = (buffer).max_size = (len))
#define noise_buffer_set_inout(buffer, ptr, len, max) \
    ((buffer).data = (ptr), (buffer).size = (len), (buffer).max_size = (max))
#endif

#ifndef NOISE_CONSTANTS_H
/* include/noise/protocol/constants.h:31-38, 131-151 */
#define NOISE_ID(ch, num) ((((int)(ch)) << 8) | ((int)(num)))
#define NOISE_CIPHER_NONE 0
#define NOISE_CIPHER_CATEGORY NOISE_ID('C', 0)
#define NOISE_CIPHER_CHACHAPOLY NOISE_ID('C', 1)
#define NOISE_CIPHER_AESGCM NOISE_ID('C', 2)
#define NOISE_PADDING_ZERO NOISE_ID('G', 1) /* constants.h:123-124 */
#define NOISE_PADDING_RANDOM NOISE_ID('G', 2)
#define NOISE_HASH_BLAKE2s NOISE_ID('H', 1) /* constants.h:43-46 */
#define NOISE_HASH_BLAKE2b NOISE_ID('H', 2)
#define NOISE_HASH_SHA256 NOISE_ID('H', 3)
#define NOISE_HASH_SHA512 NOISE_ID('H', 4)
#define NOISE_DH_CURVE25519 NOISE_ID('D', 1) /* constants.h:51 */
#define NOISE_ERROR_NONE 0
#define NOISE_ERROR_NO_MEMORY NOISE_ID('E', 1)
#define NOISE_ERROR_UNKNOWN_ID NOISE_ID('E', 2)
#define NOISE_ERROR_UNKNOWN_NAME NOISE_ID('E', 3)
#define NOISE_ERROR_MAC_FAILURE NOISE_ID('E', 4)
#define NOISE_ERROR_NOT_APPLICABLE NOISE_ID('E', 5)
#define NOISE_ERROR_SYSTEM NOISE_ID('E', 6)
#define NOISE_ERROR_INVALID_LENGTH NOISE_ID('E', 10)
#define NOISE_ERROR_INVALID_PARAM NOISE_ID('E', 11)
#define NOISE_ERROR_INVALID_STATE NOISE_ID('E', 12)
#define NOISE_ERROR_INVALID_NONCE NOISE_ID('E', 13)
#define NOISE_MAX_PAYLOAD_LEN 65535
#define NOISE_ROLE_INITIATOR NOISE_ID('R', 1) /* constants.h:111-112 */
#define NOISE_ROLE_RESPONDER NOISE_ID('R', 2)
#define NOISE_ACTION_NONE 0 /* constants.h:115-120 */
#define NOISE_ACTION_WRITE_MESSAGE NOISE_ID('A', 1)
#define NOISE_ACTION_READ_MESSAGE NOISE_ID('A', 2)
#define NOISE_ACTION_FAILED NOISE_ID('A', 3)
#define NOISE_ACTION_SPLIT NOISE_ID('A', 4)
#define NOISE_ACTION_COMPLETE NOISE_ID('A', 5)
#define NOISE_ERROR_REMOTE_KEY_REQUIRED NOISE_ID('E', 7) /* constants.h:138-140, 146 */
#define NOISE_ERROR_LOCAL_KEY_REQUIRED NOISE_ID('E', 8)
#define NOISE_ERROR_PSK_REQUIRED NOISE_ID('E', 9)
#define NOISE_ERROR_INVALID_PUBLIC_KEY NOISE_ID('E', 15)
#define NOISE_SIGN_ED25519 NOISE_ID('S', 1) /* constants.h:108, 148 */
#define NOISE_ERROR_INVALID_SIGNATURE NOISE_ID('E', 17)
#endif

/* ------------------------------------------------ 1. CipherState API
 * Each replaces the function of the same name in src/protocol/cipherstate.c.
 * Single encrypt/decrypt calls launch nothing: a resident worker workgroup
 * per calling thread (up to one per high-priority hardware queue of the
 * device, GPU_MAX_HW_QUEUES: 4 by default) serves them through a request
 * slot, ~8-12 us per record up to 1.4 KB; it leaves after 2 ms without
 * requests, when a batch launch fills the device, or when a state whose key
 * it caches is freed.  NOISE_AEAD_WORKER=0: one kernel launch per call. */

typedef struct NoiseCipherState_s NoiseCipherState;

int noise_cipherstate_new_by_id(NoiseCipherState **state, int id);        /* cipherstate.c:77-104 */
int noise_cipherstate_new_by_name(NoiseCipherState **state, const char *name); /* :122-140 */
int noise_cipherstate_free(NoiseCipherState *state);                      /* :152-165 */
int noise_cipherstate_get_cipher_id(const NoiseCipherState *state);       /* :174-177 */
size_t noise_cipherstate_get_key_length(const NoiseCipherState *state);   /* :188-191 */
size_t noise_cipherstate_get_mac_length(const NoiseCipherState *state);   /* :202-205 */
int noise_cipherstate_init_key(NoiseCipherState *state, const uint8_t *key,
                               size_t key_len);                           /* :221-235 */
int noise_cipherstate_has_key(const NoiseCipherState *state);             /* :247-250 */
int noise_cipherstate_encrypt_with_ad(NoiseCipherState *state, const uint8_t *ad,
                                      size_t ad_len, NoiseBuffer *buffer); /* :293-333 */
int noise_cipherstate_decrypt_with_ad(NoiseCipherState *state, const uint8_t *ad,
                                      size_t ad_len, NoiseBuffer *buffer); /* :373-410 */
int noise_cipherstate_encrypt(NoiseCipherState *state, NoiseBuffer *buffer); /* :452-455 */
int noise_cipherstate_decrypt(NoiseCipherState *state, NoiseBuffer *buffer); /* :494-497 */
int noise_cipherstate_set_nonce(NoiseCipherState *state, uint64_t nonce);    /* :518-535 */
int noise_cipherstate_get_max_key_length(void);                           /* :542-545 */
int noise_cipherstate_get_max_mac_length(void);                           /* :552-555 */

/* ------------------------------------------------ 2. plugin constructors
 * internal.h:655-656; objects start with struct NoiseCipherState_s
 * (internal.h:58-146) filled as cipher-chachapoly.c:145-158 /
 * cipher-aesgcm.c:190-203 do, plus a destroy hook (as the OpenSSL backend,
 * src/backend/openssl/cipher-aesgcm.c:188-204) that frees device memory. */
NoiseCipherState *noise_chachapoly_new(void);
NoiseCipherState *noise_aesgcm_new(void);

/* ------------------------------------------------ 3. batch (host buffers)
 *
 * Process count records: record i is buffers[i] under states[i] (states may
 * repeat and may mix ciphers) with associated data ads[i]/ad_lens[i] (both
 * arrays may be NULL for no AD).  results[i] receives exactly what
 *   noise_cipherstate_{en,de}crypt_with_ad(states[i], ads[i], ad_lens[i], &buffers[i])
 * would have returned had the calls been made one by one in index order, and
 * buffers, sizes and nonces end up exactly as after those calls (including
 * the no-key pass-through, nonce exhaustion and the "nonce not advanced on a
 * MAC failure" rule, cipherstate.c:321-326, 400-405).  One GPU pass in the
 * common case.  Returns NOISE_ERROR_NONE unless an argument is invalid or the
 * GPU fails (NOISE_ERROR_SYSTEM; then results[] is unspecified). */
int noise_cipherstate_encrypt_batch(NoiseCipherState *const *states,
                                    const uint8_t *const *ads, const size_t *ad_lens,
                                    NoiseBuffer *buffers, size_t count, int *results);
int noise_cipherstate_decrypt_batch(NoiseCipherState *const *states,
                                    const uint8_t *const *ads, const size_t *ad_lens,
                                    NoiseBuffer *buffers, size_t count, int *results);

/* ------------------------------------------------ 3b. transport wire buffers
 *
 * SURVEY.md §8f rank 1.  A wire buffer holds frames in the format of the
 * reference's examples/echo (echo-common.c:643-688, echo_recv/echo_send):
 * a 2-byte big-endian length L, then L bytes of CT || tag.  These calls work
 * in place on every complete frame at the start of the buffer, frame k under
 * nonce n + k of its CipherState, in one pipelined GPU pass:
 *
 *   noise_wire_seal : each frame holds L - 16 bytes of plaintext followed by
 *                     16 bytes of room; they become CT || tag.  The header is
 *                     already the final length (what echo_send writes).
 *   noise_wire_open : each frame's first L - 16 bytes become its plaintext
 *                     (the 16 tag bytes after it are left as they were).
 *   noise_wire_echo : the echo server's transport loop (echo-server.c
 *                     :377-407): every frame opened with `recv` and sealed
 *                     again with `send` (same length, so in place).
 *
 * *frames / *consumed report the frames processed and the bytes they span.
 * Processing stops, exactly as the per-frame CipherState calls would, at:
 *   - a partial frame at the end (returns NOISE_ERROR_NONE);
 *   - a frame with L < 16 (NOISE_ERROR_INVALID_LENGTH) or an exhausted
 *     nonce (NOISE_ERROR_INVALID_NONCE) — that frame is untouched;
 *   - open/echo: the first frame whose tag fails (NOISE_ERROR_MAC_FAILURE):
 *     it and every later frame are untouched and n stays at its nonce, the
 *     rule of cipherstate.c:400-405 applied frame by frame.
 * Nonces advance by the frames processed (seal: by every frame dispatched,
 * also on NOISE_ERROR_SYSTEM, as cipherstate.c:325-326).  The states must be
 * keyed (NOISE_ERROR_INVALID_STATE otherwise) and, for echo, distinct.
 *
 * Buffers from noise_wire_alloc() are pinned host memory: H2D and D2H use
 * them directly.  Any other buffer is staged through pinned memory. */
void *noise_wire_alloc(size_t bytes);
void noise_wire_free(void *wire);
int noise_wire_seal(NoiseCipherState *state, uint8_t *wire, size_t wire_len,
                    size_t *consumed, size_t *frames);
int noise_wire_open(NoiseCipherState *state, uint8_t *wire, size_t wire_len,
                    size_t *consumed, size_t *frames);
int noise_wire_echo(NoiseCipherState *recv, NoiseCipherState *send, uint8_t *wire,
                    size_t wire_len, size_t *consumed, size_t *frames);

/* ------------------------------------------------ 4. device-resident API
 *
 * All pointers below are device pointers on the current HIP device; `stream`
 * is a hipStream_t (NULL = default stream).  Calls are asynchronous.
 *
 * Key contexts: n_states contexts of noise_aead_dev_ctx_bytes(cipher) bytes
 * each, built from n_states raw 32-byte keys by noise_aead_dev_prepare
 * (ChaChaPoly: the key itself; AESGCM: round keys + GHASH tables). */
size_t noise_aead_dev_ctx_bytes(int cipher_id);
int noise_aead_dev_prepare(int cipher_id, const uint8_t *d_raw_keys, uint32_t n_states,
                           void *d_ctx, void *stream);

/* Uniform batch.  Record i (0 <= i < n_records) belongs to state
 * s = i / recs_per_state and uses nonce nonce_base[s] + i % recs_per_state.
 * seal: in + i*in_stride holds len plaintext bytes; out + i*out_stride
 *       receives CT || tag (len + 16 bytes).
 * open: in + i*in_stride holds CT || tag; status[i] = 0 (ok) or 1 (MAC
 *       failure).  A verified record's len plaintext bytes go to
 *       out + i*out_stride.  Open order:
 *         - AESGCM opens always authenticate first and write a record's
 *           output only after its tag verified — the order of the
 *           reference's ref backends (cipher-aesgcm.c:172-188): a rejected
 *           record's output is not written at all (in place: CT || tag read
 *           back as given; out of place: the output bytes keep whatever
 *           they held).  It costs nothing there.
 *         - CHACHAPOLY opens take the same order by default (round 6; the
 *           reference's cipher-chachapoly.c:135-141): authenticate, then
 *           decrypt and write only verified records.  With the opt-in
 *           NOISE_AEAD_FLAG_ONE_PASS a FAST-layout ChaChaPoly open decrypts
 *           as it authenticates (one pass over the ciphertext, DESIGN.md
 *           4.1b gives the rate difference), and a rejected record reads
 *           back in place exactly as given, out of place as ZEROED output
 *           bytes; until the kernel ends its output bytes may transiently
 *           hold unauthenticated plaintext, which the kernel undoes
 *           (restores / zeroes) before it completes.
 * Memory: input and output records must be either exactly in place
 * (in == out and in_stride == out_stride) or disjoint record by record:
 * with one stride for both sides the records may interleave (input and
 * output slots alternating in one buffer) as long as no input record
 * [in + i*stride, + len (+16 open)) meets an output record; with two
 * strides the two spans must be disjoint.  Anything else is refused with
 * NOISE_ERROR_INVALID_PARAM.
 * lanes_per_record: 0 = automatic; ChaChaPoly 1, 2, 4, 8, 16, 32 or 64 (wider
 * groups cut the latency of small batches of long records); AESGCM 4 (0 lets
 * a ragged batch of at most 512 records run one record per workgroup). */
typedef struct NoiseAeadUniform {
    const void *ctx;
    const uint64_t *nonce_base;
    const uint8_t *in;
    uint8_t *out;
    const uint8_t *ad;       /* may be NULL when ad_len == 0 */
    uint8_t *status;         /* open only; may be NULL */
    uint64_t in_stride, out_stride, ad_stride;
    uint32_t recs_per_state;
    uint32_t n_records;
    uint32_t len;            /* <= 65535 - 16 */
    uint32_t ad_len;
    uint32_t lanes_per_record;
    uint32_t flags;          /* NOISE_AEAD_FLAG_CT_GHASH, _VERIFY_FIRST, _ONE_PASS (FAST is derived) */
} NoiseAeadUniform;

int noise_aead_dev_seal_uniform(int cipher_id, const NoiseAeadUniform *job, void *stream);
int noise_aead_dev_open_uniform(int cipher_id, const NoiseAeadUniform *job, void *stream);

/* Duplex: seal_job and open_job in one launch — an echo server's two
 * directions (echo-server.c:377-407 opens what it receives and seals what it
 * sends) or a pipeline sealing one batch while opening an earlier one.  The
 * result is exactly noise_aead_dev_seal_uniform(seal_job) followed by
 * noise_aead_dev_open_uniform(open_job); the jobs must be independent:
 * nothing one job writes (its output records, the open job's statuses) may
 * overlap anything the other job reads (records, AD) or writes, else
 * NOISE_ERROR_INVALID_PARAM.  Either job may have n_records == 0.  When the
 * two jobs cannot share a kernel (unaligned layouts, different lane counts,
 * AESGCM without one state per 256 records, a VERIFY_FIRST ChaChaPoly open
 * on 4 or 8 lanes per record) the library issues the two launches on
 * `stream` instead; a verify-first open (the default) on one lane per record
 * (the default from 65 536 records) or on the staged AES-GCM kernel keeps the
 * one launch. */
int noise_aead_dev_duplex_uniform(int cipher_id, const NoiseAeadUniform *seal_job,
                                  const NoiseAeadUniform *open_job, void *stream);

/* Ragged batch: one descriptor per record.  The key context of a record is
 * at ctx_base + ctx_off (ctx_base may be NULL with absolute ctx_off). */
typedef struct NoiseAeadRecord {
    uint64_t in_off;
    uint64_t out_off;
    uint64_t nonce;
    uint64_t ctx_off;
    uint64_t ad_off;
    uint32_t len;
    uint32_t ad_len;
} NoiseAeadRecord;

typedef struct NoiseAeadRagged {
    const void *ctx_base;
    const NoiseAeadRecord *recs; /* device array of n_records descriptors */
    const uint8_t *in;
    uint8_t *out;
    const uint8_t *ad;
    uint8_t *status;
    uint32_t n_records;
    uint32_t lanes_per_record;
    uint32_t flags;              /* NOISE_AEAD_FLAG_* */
    uint32_t reserved_;
} NoiseAeadRagged;

/* A record longer than NOISE_MAX_PAYLOAD_LEN - 16 (65519) bytes is not
 * processed: nothing is written and, when status is given, status[i] = 2 —
 * for seal too (status is optional there: 0 sealed, 2 refused).
 *
 * Open: a rejected record's output is handled as for the uniform open (not
 * written at all by default; restored in place / zeroed out of place under
 * NOISE_AEAD_FLAG_ONE_PASS).  Each record's input and output ranges must
 * be identical (in + in_off == out + out_off) or disjoint from every other
 * record's ranges; the descriptors live in device memory, so this is the
 * caller's guarantee (not checked).
 *
 * The caller guarantees, for every record: in + in_off and out + out_off are
 * 16-byte aligned, and the input may be read up to roundup64(max(len, 1))
 * bytes (and holds CT || tag for open).  Enables the straight-line dwordx4 path.  The
 * uniform API derives this itself from the pointers and strides. */
#define NOISE_AEAD_FLAG_FAST 1u

/* AESGCM only: GHASH without lookup tables.  The default GHASH multiplies
 * by H through 4-bit tables indexed by the running hash (LDS copies are
 * bank-conflict-free; the per-lane final scale reads the context's tables in
 * global memory, whose cache-line footprint depends on secret data).  With
 * this flag every multiply is a carry-less 128x128 product built from integer
 * multiplies of masked operands (no secret-dependent address or branch) —
 * slower; DESIGN.md §4 gives both throughputs.  Setting the environment
 * variable NOISE_AEAD_CT_GHASH=1 before the first call turns it on for every
 * job, including the CipherState and wire paths. */
#define NOISE_AEAD_FLAG_CT_GHASH 2u

/* Open only: authenticate first, decrypt only a verified record, and write
 * nothing for a rejected one (the reference's verify-then-decrypt order,
 * cipher-chachapoly.c:135-141, cipher-aesgcm.c:172-188).  Since round 6
 * this is the order of every open whether or not the flag is set; the flag
 * stays accepted, and it overrides NOISE_AEAD_FLAG_ONE_PASS. */
#define NOISE_AEAD_FLAG_VERIFY_FIRST 4u

/* Open only, ChaChaPoly FAST layouts, opt-in: decrypt while authenticating
 * (one pass over the ciphertext) and undo a rejected record's plaintext
 * before the kernel ends — restored in place, zeroed out of place (see the
 * uniform open above).  Faster on the device API; the
 * host paths (CipherState API, batch, wire) never set it.  AESGCM opens and
 * non-FAST layouts ignore it (they always verify first). */
#define NOISE_AEAD_FLAG_ONE_PASS 8u

int noise_aead_dev_seal_ragged(int cipher_id, const NoiseAeadRagged *job, void *stream);
int noise_aead_dev_open_ragged(int cipher_id, const NoiseAeadRagged *job, void *stream);

/* Ragged duplex: seal_job and open_job in one launch per call where the two
 * can share a kernel — an echo server's or proxy's tick: a batch of received
 * frames to open and a batch of outgoing frames to seal, across many
 * sessions, in every length.  The result is exactly
 * noise_aead_dev_seal_ragged(seal_job) followed by
 * noise_aead_dev_open_ragged(open_job) on `stream`: every byte of both
 * outputs, both status arrays (the seal job's optional one: 0 or 2) and
 * every byte the separate calls leave untouched.
 *
 * Each job keeps its own flags and lanes_per_record with the meaning they
 * have above: FAST is the caller's guarantee per job, the open verifies
 * first unless NOISE_AEAD_FLAG_ONE_PASS is set (honoured for FAST ChaChaPoly
 * opens exactly as noise_aead_dev_open_ragged honours it),
 * NOISE_AEAD_FLAG_CT_GHASH works per job, and a record over 65519 bytes gets
 * status 2 and nothing written.  Each job must be a valid ragged job (else
 * NOISE_ERROR_INVALID_PARAM); a job with n_records == 0 is valid and leaves
 * the call equal to the other job's standalone call.  An unknown cipher
 * gives NOISE_ERROR_UNKNOWN_ID.
 *
 * The jobs must be independent: nothing one job writes (its output records,
 * its statuses) may meet anything the other job reads (records, AD) or
 * writes.  The descriptors live in device memory, so for the record and AD
 * ranges this is the caller's guarantee (not checked, as for the ragged
 * calls above); the two status arrays are checked: if both are given and
 * [status, status + n_records) of the two meet, the call is refused with
 * NOISE_ERROR_INVALID_PARAM and nothing is written.
 *
 * The launch is shared when both jobs, each planned alone, take the same
 * kernel family with the same template arguments: two segmented ChaChaPoly
 * jobs (FAST, automatic lanes, 16384 records or more each), two windowed
 * ChaChaPoly jobs on the same lanes per record and the same FAST, two
 * windowed AES-GCM jobs of the same launch shape, FAST and CT_GHASH.
 * Otherwise (a small AES-GCM job with automatic lanes, different lane
 * counts or shapes, one segmented and one windowed job, FAST on one AES-GCM
 * job only) the library issues the two launches on `stream`, seal first.
 * NOISE_AEAD_RAGGED_DUPLEX=0 in the environment (read once) makes every
 * ragged duplex two launches, =1 shares wherever the jobs agree; unset, a
 * family shares by default where that was measured faster. */
int noise_aead_dev_duplex_ragged(int cipher_id, const NoiseAeadRagged *seal_job,
                                 const NoiseAeadRagged *open_job, void *stream);

/* ------------------------------------------------ 5. session key fan-out
 *
 * SURVEY.md §8f rank 2.  For n sessions at once, the HKDF of
 * noise_hashstate_hkdf (src/protocol/hashstate.c:476-516) with the session's
 * Noise hash (NOISE_HASH_BLAKE2s/BLAKE2b/SHA256/SHA512):
 *   out1[i] || out2[i] = HKDF(keys[i], data[i])   (each truncated)
 * keys[i] = d_keys + i*key_len (1..256 bytes), data[i] = d_data + i*data_len
 * (0..256 bytes; d_data may be NULL when data_len is 0), output lengths at
 * most the hash length (NOISE_ERROR_INVALID_LENGTH otherwise, as
 * hashstate.c:496-497).  noise_aead_dev_split is the key derivation of
 * noise_symmetricstate_split (symmetricstate.c:530-533): HKDF(ck, "") into
 * two 32-byte transport keys per session (ck is the hash length), ready for
 * noise_aead_dev_prepare.  Device pointers, asynchronous on `stream`. */
int noise_aead_dev_hkdf(int hash_id, const uint8_t *d_keys, uint32_t key_len,
                        const uint8_t *d_data, uint32_t data_len, uint32_t n, uint8_t *d_out1,
                        uint32_t out1_len, uint8_t *d_out2, uint32_t out2_len, void *stream);
int noise_aead_dev_split(int hash_id, const uint8_t *d_ck, uint32_t n, uint8_t *d_k1,
                         uint8_t *d_k2, void *stream);

/* Handshake-payload AEAD for a batch of SymmetricStates (SURVEY.md §8f
 * rank 3): noise_symmetricstate_encrypt_and_hash / decrypt_and_hash
 * (symmetricstate.c:352-445) on n keyed states at once.  d_h holds the n
 * handshake hashes (hash-length bytes each); the job's AD must be those
 * hashes: job->ad == d_h and record i's ad_off = i * hash_len, ad_len =
 * hash_len.  Encrypt seals record i with AD = h_i, then
 * h_i = HASH(h_i || CT_i || tag_i).  Decrypt hashes CT_i || tag_i first,
 * opens, and keeps the new h_i only where status[i] == 0 (the reference
 * leaves h unchanged on a MAC failure, :425-443); job->status is required. */
int noise_aead_dev_encrypt_and_hash(int cipher_id, int hash_id, uint8_t *d_h,
                                    const NoiseAeadRagged *job, void *stream);
int noise_aead_dev_decrypt_and_hash(int cipher_id, int hash_id, uint8_t *d_h,
                                    const NoiseAeadRagged *job, void *stream);

/* ------------------------------------------------ 6. batched padding
 *
 * SURVEY.md §8f rank 4.  n calls of noise_randstate_pad(state, payload_i,
 * orig_lens[i], padded_len, padding_mode) (randstate.c:348-375) in record
 * order, payload_i = d_payloads + i*stride, so that messages padded to one
 * length (echo-client -g, echo-client.c:400-410) go through
 * noise_aead_dev_seal_uniform.  A record with padded_len <= orig_lens[i] is
 * left alone and does not touch the generator.
 *  - NOISE_PADDING_ZERO: the padding bytes are zeroed.
 *  - NOISE_PADDING_RANDOM (and, as in the reference, any unknown mode): the
 *    bytes of noise_randstate_generate (:263-316) drawn from *d_rand, a device
 *    copy of the RandState generator (its ChaCha key, 64-bit block counter,
 *    64-bit IV and reseed budget `left`, randstate.c:47-58), advanced in place
 *    exactly as the sequential calls advance it (rekeys included).  When a
 *    call would need a reseed from OS entropy (left too small) the walk stops
 *    before that record: records from there on are untouched and *d_done
 *    (optional) = records processed — the caller reseeds and calls again.
 *  - d_rand == NULL: the padding is zeroed and NOISE_ERROR_INVALID_PARAM is
 *    returned (the reference's NULL-state rule).
 * Device pointers, asynchronous on `stream`. */
typedef struct NoiseRandSnapshot {
    uint32_t key[8];
    uint64_t counter;
    uint64_t iv;
    uint64_t left;
} NoiseRandSnapshot;

int noise_aead_dev_pad(NoiseRandSnapshot *d_rand, uint8_t *d_payloads, uint64_t stride,
                       const uint32_t *d_orig_lens, uint32_t padded_len, uint32_t n,
                       int padding_mode, uint32_t *d_done, void *stream);

/* ------------------------------------------------ 7. batched X25519
 *
 * n calls of noise_dhstate_calculate for Curve25519 (src/protocol/dhstate.c
 * :685-717, which runs curve25519_donna, src/backend/ref/dh-curve25519.c
 * :94-103) in one launch, so that DH -> mix_key (noise_aead_dev_hkdf) ->
 * split -> prepare -> seal runs for n sessions without a host round trip.
 * Session i multiplies the 32-byte private key at d_priv + i*priv_stride by
 * the 32-byte public value at d_pub + i*pub_stride and writes the 32-byte
 * shared key at d_shared + 32*i: packed, directly the d_data of
 * noise_aead_dev_hkdf(..., data_len = 32, ...).  A stride of 0 is one key for
 * all n sessions (a server's static key against n client ephemerals, the
 * es / se tokens); any other stride must be at least 32.  No pointer or
 * stride needs any alignment.
 *
 * Byte for byte what the reference computes: the private key is clamped
 * inside the call (the keys in memory are never written), bit 255 of the
 * public value is ignored, a public value of 2^255 - 19 or more is accepted
 * and reduced, the result is fully reduced.  The all-zero public value gives
 * the all-zero shared key (the reference's null rule, dhstate.c:702-715, which
 * the arithmetic satisfies by itself), and so does every other point of small
 * order, without an error (dh-curve25519.c:99-102).
 * noise_aead_dev_dh_public is curved25519_scalarmult_basepoint
 * (dh-curve25519.c:49,73) for n private keys: the same ladder on u = 9, which
 * also clamps; public key i goes to d_pub_out + 32*i.
 *
 * Constant time: 255 ladder steps whatever the key, swaps by mask, no branch,
 * address or table index that depends on a key bit or an intermediate value
 * (the base point takes the ladder too), and no scratch memory: no limb of a
 * key or of an intermediate is spilled to device memory.
 *
 * Checked on the host before any launch: dh_id other than NOISE_DH_CURVE25519
 * gives NOISE_ERROR_UNKNOWN_ID; n == 0 gives NOISE_ERROR_NONE and touches
 * nothing; otherwise a NULL pointer, a stride in 1..31, or an output range
 * [d_shared, + 32 n) that meets an input span ([ptr, + (n - 1)*stride + 32))
 * gives NOISE_ERROR_INVALID_PARAM, with nothing written.
 * Device pointers, asynchronous on `stream`. */
int noise_aead_dev_dh_calculate(int dh_id, const uint8_t *d_priv, uint64_t priv_stride,
                                const uint8_t *d_pub, uint64_t pub_stride, uint32_t n,
                                uint8_t *d_shared, void *stream);
int noise_aead_dev_dh_public(int dh_id, const uint8_t *d_priv, uint64_t priv_stride, uint32_t n,
                             uint8_t *d_pub_out, void *stream);

/* ------------------------------------------------ 8. batched handshakes
 *
 * n Noise handshakes of one protocol and one role, run message by message
 * without a host round trip: what noise_handshakestate_start / _write_message
 * / _read_message / _split (src/protocol/handshakestate.c:800-885, 1151-1340,
 * 1419-1600; symmetricstate.c:97-108, 514-573) do for one session, done for
 * session i of the batch alone.  An opaque host object owns the device state
 * (ck, h, k, key contexts, descriptors, a DH arena, statuses, local public
 * keys, remote e and s: all allocated by _new; a message call allocates
 * nothing).  Every data pointer is a device pointer; every call is
 * asynchronous on `stream`, and none synchronises or copies to the host.  The
 * calls of one object must be issued in stream order (one stream, or streams
 * the caller orders).
 *
 * In scope: the patterns N K X NN NK NX XN XK XX KN KK KX IN IK IX over
 * Curve25519, ChaChaPoly or AESGCM, the four hashes, the prefixes "Noise" and
 * "NoisePSK" (the reference's old-style PSK: after the prologue ck, temp =
 * HKDF(ck, psk) and MixHash(temp), handshakestate.c:833-842; every `e` token
 * also MixKey(e.public), :1214-1217, :1477-1481).  A name that parses but
 * needs Curve448, NewHope, a hybrid ("hfs") pattern or XXfallback gives
 * NOISE_ERROR_NOT_APPLICABLE; anything else that is not a protocol name gives
 * NOISE_ERROR_UNKNOWN_NAME.
 *
 * Strides: session i's value is at pointer + i * stride.  A stride of 0 is one
 * value for all sessions (a server's static key, a shared prologue, one
 * payload for all); any other key stride must be at least 32, any other
 * prologue, payload or message stride at least the length; an output stride
 * must be at least the bytes written (never 0).  Nothing needs alignment.
 * Payload and message lengths are uniform over the batch in
 * _write_message / _read_message; the _ragged calls below take both the place
 * and the length per session.
 *
 * _new consumes the prologue, the PSK and the remote static public keys; the
 * private keys (d_local_static_priv, d_local_ephemeral_priv) are read by
 * later calls and must stay valid and unchanged until the split.  The
 * ephemeral private keys are the caller's entropy, fresh per session, as the
 * reseed of noise_aead_dev_pad is.  Start-up is the reference's: h = the name
 * zero-padded to the hash length, or HASH(name) when longer; ck = h; then
 * MixHash(prologue) (the empty one too, :826-829), the PSK step, and MixHash
 * of the initiator's pre-message static key, then of the responder's
 * (:844-877).
 *
 * Messages: _get_action says which call is next (an initiator starts with
 * NOISE_ACTION_WRITE_MESSAGE, a responder with _READ_MESSAGE; after the last
 * message — for a one-way pattern its only one — NOISE_ACTION_SPLIT, after
 * the split _COMPLETE).  _overhead is what the next message adds to its
 * payload: 32 per `e`, 32 per `s` plus 16 once a key is set (:1487-1488), 16
 * for the payload once a key is set.  write_message builds
 * d_msg + i * msg_stride from d_payload + i * payload_stride (payload_len
 * bytes; d_payload may be NULL when 0) and writes payload_len + overhead
 * bytes; read_message takes msg_len bytes and writes msg_len - overhead
 * payload bytes to d_payload + i * payload_stride.  Before the first MixKey
 * encrypt_and_hash / decrypt_and_hash pass the bytes through and MixHash them;
 * the nonce restarts at 0 on every MixKey and counts one per AEAD.
 * _split writes k1[i], k2[i] = HKDF(ck_i, "") truncated to 32 bytes, packed 32
 * bytes apart in the order of noise_aead_dev_split (the initiator sends under
 * k1), ready for noise_aead_dev_prepare, and h_i (hash-length bytes apart) to
 * d_handshake_hash when it is not NULL.
 *
 * Checked on the host before any launch, in this order:
 *   - the wrong call for _get_action: NOISE_ERROR_INVALID_STATE;
 *   - _new without a key the pattern needs of this role:
 *     NOISE_ERROR_LOCAL_KEY_REQUIRED (static or ephemeral private key),
 *     NOISE_ERROR_REMOTE_KEY_REQUIRED, NOISE_ERROR_PSK_REQUIRED (d_psk is
 *     required with NoisePSK and ignored otherwise);
 *   - a message over 65535 bytes, or msg_len below the overhead:
 *     NOISE_ERROR_INVALID_LENGTH;
 *   - a NULL pointer, a stride in 1..31 (keys) or below the length, an output
 *     stride that is too short, or an output span
 *     [out, out + (n - 1) * stride + bytes) that meets the input span of the
 *     same call (split: two outputs that meet): NOISE_ERROR_INVALID_PARAM.
 * n == 0 gives a valid object whose calls check the state and the lengths,
 * launch nothing and advance the action.
 *
 * Per-session offsets and lengths: _write_message_ragged and
 * _read_message_ragged are _write_message and _read_message done for session
 * i with its own place and length — the same tokens, bytes, nonce and status
 * rules.  Session i's payload is the d_payload_len[i] bytes at d_payload +
 * d_payload_off[i], its message lies at d_msg + d_msg_off[i]; the offset and
 * length arrays are device arrays of n entries, as in section 9.  Nothing
 * needs alignment and the offsets may come in any order.  On write
 * d_payload, d_payload_off and d_payload_len may be NULL all three together:
 * every payload is then empty.  Write sets d_msg_len[i] = d_payload_len[i] +
 * overhead, read sets d_payload_len[i] = d_msg_len[i] - overhead; either is
 * 0 for every session whose status is non-zero after the call.  The spans
 * are the caller's guarantee, unchecked, as for the ragged calls of section
 * 4 and the transport: each output span has room (payload length + overhead
 * on write, message length - overhead on read) and no output span meets any
 * span of the same call.  _get_action and _overhead stay host values, the
 * action advances for the batch regardless, and uniform and ragged calls may
 * be mixed freely within one handshake.  What the uniform calls refuse for
 * the whole batch as NOISE_ERROR_INVALID_LENGTH becomes status 4 of the one
 * session: a write with payload length + overhead > 65535, a read with
 * message length < overhead or > 65535.  The length is checked before any
 * token (the reference gives the same code at the token it reaches,
 * :1454, :1489, :1320-1324, symmetricstate.c:419-422, and is
 * NOISE_ACTION_FAILED afterwards), so such a session is a failed session
 * from the start of the call.  The order of causes within one call for one
 * session: already failed, then the length (4), then a null ephemeral (3),
 * then a tag (1).  Checked on the host before any launch, in this order:
 *   - hs == NULL: NOISE_ERROR_INVALID_PARAM;
 *   - the wrong call for _get_action: NOISE_ERROR_INVALID_STATE;
 *   - n == 0: NOISE_ERROR_NONE, nothing is launched, the action advances;
 *   - a NULL pointer other than the write's payload triple all together, or
 *     only part of that triple NULL: NOISE_ERROR_INVALID_PARAM;
 *   - the output length array [out, out + 4n) meeting an input offset array
 *     [p, p + 8n) or the input length array [p, p + 4n):
 *     NOISE_ERROR_INVALID_PARAM.
 * A refused call leaves the object as it was.
 *
 * Per-session failures stay on the device: status[i] is 0 (ok), 1 (a tag
 * failed: NOISE_ERROR_MAC_FAILURE), 3 (the received ephemeral was all-zero:
 * NOISE_ERROR_INVALID_PUBLIC_KEY, :1464-1470) or 4 (a length a ragged call
 * refuses: NOISE_ERROR_INVALID_LENGTH); 2 stays reserved as in the
 * ragged calls; 5 is the fallback's "not in this object" (section 15); 6 is
 * never written by a handshake call: it is section 17's "signature refused:
 * NOISE_ERROR_INVALID_SIGNATURE", which noise_aead_dev_sign_verify merges into
 * a copy of these bytes or into the bytes themselves.  The
 * first failure is sticky.  A failed session writes only
 * inside its own slots and its later output bytes are unspecified; its opens
 * never write unauthenticated plaintext (the verify-first order) and nothing
 * more is sealed, opened or passed through for it; the split writes zeros for
 * its two keys.  Every other session is unaffected, byte for byte, and the
 * host action advances for the batch regardless.
 *
 * _free scrubs every device array the object owns before freeing it (it
 * waits for the device to do so), at any point of the handshake.  _status is
 * the n status bytes, _remote_static the n x 32 remote static public keys
 * (given to _new or received in an `s` token); both are device pointers owned
 * by the object. */
typedef struct NoiseAeadDevHandshake NoiseAeadDevHandshake;
typedef struct NoiseAeadHandshakeConfig {
    const char *protocol_name;   /* "Noise_XX_25519_ChaChaPoly_BLAKE2s", "NoisePSK_IK_25519_AESGCM_SHA512", ... */
    int role;                    /* NOISE_ROLE_INITIATOR / NOISE_ROLE_RESPONDER */
    uint32_t n;
    const uint8_t *d_prologue;  uint64_t prologue_stride; uint32_t prologue_len;
    const uint8_t *d_psk;       uint64_t psk_stride;       /* 32 bytes each */
    const uint8_t *d_local_static_priv;    uint64_t local_static_stride;
    const uint8_t *d_local_ephemeral_priv; uint64_t local_ephemeral_stride;
    const uint8_t *d_remote_static_pub;    uint64_t remote_static_stride;
} NoiseAeadHandshakeConfig;

int noise_aead_dev_handshake_new(NoiseAeadDevHandshake **hs, const NoiseAeadHandshakeConfig *cfg, void *stream);
int noise_aead_dev_handshake_free(NoiseAeadDevHandshake *hs);
int noise_aead_dev_handshake_get_action(const NoiseAeadDevHandshake *hs);
size_t noise_aead_dev_handshake_overhead(const NoiseAeadDevHandshake *hs);
int noise_aead_dev_handshake_write_message(NoiseAeadDevHandshake *hs, const uint8_t *d_payload,
                                           uint64_t payload_stride, uint32_t payload_len, uint8_t *d_msg,
                                           uint64_t msg_stride, void *stream);
int noise_aead_dev_handshake_read_message(NoiseAeadDevHandshake *hs, const uint8_t *d_msg, uint64_t msg_stride,
                                          uint32_t msg_len, uint8_t *d_payload, uint64_t payload_stride,
                                          void *stream);
int noise_aead_dev_handshake_write_message_ragged(NoiseAeadDevHandshake *hs, const uint8_t *d_payload,
                                                  const uint64_t *d_payload_off, const uint32_t *d_payload_len,
                                                  uint8_t *d_msg, const uint64_t *d_msg_off,
                                                  uint32_t *d_msg_len /* out */, void *stream);
int noise_aead_dev_handshake_read_message_ragged(NoiseAeadDevHandshake *hs, const uint8_t *d_msg,
                                                 const uint64_t *d_msg_off, const uint32_t *d_msg_len,
                                                 uint8_t *d_payload, const uint64_t *d_payload_off,
                                                 uint32_t *d_payload_len /* out */, void *stream);
int noise_aead_dev_handshake_split(NoiseAeadDevHandshake *hs, uint8_t *d_k1, uint8_t *d_k2,
                                   uint8_t *d_handshake_hash, void *stream);
const uint8_t *noise_aead_dev_handshake_status(const NoiseAeadDevHandshake *hs);
const uint8_t *noise_aead_dev_handshake_remote_static(const NoiseAeadDevHandshake *hs);

/* ------------------------------------------------ 9. device-resident transport sessions
 *
 * The transport phase of n Noise sessions without a host round trip: what
 * noise_wire_seal / _open / _echo (section 3b) do for one pair of
 * CipherStates, done for session i of the batch alone, in one call for all
 * sessions.  An opaque host object owns the device state: a send and a
 * receive key context and a send and a receive nonce per session, and what a
 * call needs (descriptors and statuses for max_frames records, twice the
 * descriptors for an echo, per-session counts and bases, scan scratch), all
 * allocated by _new.  A message call allocates nothing, copies nothing to the
 * host and never synchronises.  Every data pointer is a device pointer; every
 * call is asynchronous on `stream`; the calls of one object must be issued in
 * stream order (one stream, or streams the caller orders).
 *
 * _new takes the two packed arrays of n 32-byte keys exactly as
 * noise_aead_dev_handshake_split / noise_aead_dev_split write them and builds
 * the contexts with noise_aead_dev_prepare: the initiator sends under k1 and
 * receives under k2, the responder sends under k2 and receives under k1.
 * All 2n nonces start at 0.  The keys are consumed: the caller may scrub them
 * once `stream` has passed the call.  _free scrubs every device array the
 * object owns before freeing it (it waits for the device to do so), at any
 * point.  _nonces returns the object's device array of n nonces of one
 * direction (0 send, 1 receive; NULL for anything else, and for n == 0): that
 * array is the state, and a caller may read or write it in stream order — the
 * batch form of noise_cipherstate_set_nonce.
 *
 * A call: session i's stream is the d_len[i] bytes at d_wire + d_off[i]
 * (no alignment needed; d_len[i] may be 0), holding frames in the format of
 * section 3b: a 2-byte big-endian L, then L bytes.  The streams of different
 * sessions are disjoint; the offsets live in device memory, so this is the
 * caller's guarantee (not checked, as for the ragged calls).  For each
 * session alone the result is that of noise_wire_seal / _open / _echo on that
 * stream with that session's states:
 *   - frames are taken in order from the start of the stream, frame k under
 *     nonce[i] + k;
 *   - the walk stops at a partial frame with NOISE_ERROR_NONE, at a complete
 *     frame with L < 16 with NOISE_ERROR_INVALID_LENGTH, and where
 *     nonce + k == 2^64 - 1 with NOISE_ERROR_INVALID_NONCE (an echo: where
 *     either direction runs out; both directions advance by the same k).  The
 *     stopping frame and everything after it are untouched;
 *   - seal_frames: each walked frame's L - 16 plaintext bytes and 16 bytes of
 *     room become CT || tag; the send nonce advances by `frames`;
 *   - open_frames: the opens verify first.  A frame that verifies becomes its
 *     plaintext in place (its 16 tag bytes are left as they were).  At the
 *     first frame whose tag fails, error = NOISE_ERROR_MAC_FAILURE (it wins
 *     over a later stop code), frames and consumed cover the verified prefix
 *     only, the receive nonce advances by that prefix and stays at the failed
 *     frame's nonce (nothing is sticky: cipherstate.c:400-405), and the failed
 *     frame is byte for byte untouched;
 *   - echo_frames: the open under the receive state, then the seal of the
 *     verified prefix only under the send state, in place; result and both
 *     nonces as for the open.
 * Unlike noise_wire_open, a walked frame AFTER the failed one in the same call
 * is not read back as given: it holds either its bytes as given or its
 * plaintext, the latter when its own tag verified under nonce + k — never
 * anything else and never unauthenticated plaintext.  result.frames says what
 * is valid.  (Reading them back as given would cost a restoring launch per
 * call.)
 *
 * The cap: the walked frames of a call are numbered across the batch in
 * session order (session 0's first, then session 1's, ...), in 64 bits.  A
 * frame whose number is max_frames or more is not processed in this call:
 * its session reports the frames before it with NOISE_ERROR_NONE (it did not
 * reach its stop), later sessions report 0 frames, 0 bytes and
 * NOISE_ERROR_NONE; the caller adds `consumed` to its offsets (and takes it
 * from its lengths) and calls again.  One session's failure or stop changes
 * nothing, byte for byte, for any other session.
 *
 * Checked on the host before any launch, in this order:
 *   - _new: a cipher other than NOISE_CIPHER_CHACHAPOLY / _AESGCM gives
 *     NOISE_ERROR_UNKNOWN_ID; a role that is neither NOISE_ROLE_INITIATOR nor
 *     _RESPONDER, a NULL tr, d_k1 or d_k2, and, with n > 0, max_frames == 0
 *     or over 2^31 give NOISE_ERROR_INVALID_PARAM;
 *   - a call: a NULL tr, d_wire, d_off, d_len or d_result, and
 *     [d_result, + 16 n) meeting [d_off, + 8 n) or [d_len, + 4 n), give
 *     NOISE_ERROR_INVALID_PARAM.
 * n == 0 gives a valid object whose calls launch nothing. */
typedef struct NoiseAeadDevTransport NoiseAeadDevTransport;
typedef struct NoiseAeadTransportResult {
    uint32_t frames;    /* frames of this session processed by the call */
    uint32_t consumed;  /* bytes they span, headers included */
    int32_t  error;     /* NOISE_ERROR_NONE / _INVALID_LENGTH / _INVALID_NONCE / _MAC_FAILURE */
    uint32_t reserved_; /* written as 0 */
} NoiseAeadTransportResult;

int noise_aead_dev_transport_new(NoiseAeadDevTransport **tr, int cipher_id, int role, uint32_t n,
                                 const uint8_t *d_k1, const uint8_t *d_k2, uint32_t max_frames, void *stream);
int noise_aead_dev_transport_free(NoiseAeadDevTransport *tr);
uint64_t *noise_aead_dev_transport_nonces(const NoiseAeadDevTransport *tr, int direction); /* 0 send, 1 receive */
int noise_aead_dev_transport_seal_frames(NoiseAeadDevTransport *tr, uint8_t *d_wire, const uint64_t *d_off,
                                         const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream);
int noise_aead_dev_transport_open_frames(NoiseAeadDevTransport *tr, uint8_t *d_wire, const uint64_t *d_off,
                                         const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream);
int noise_aead_dev_transport_echo_frames(NoiseAeadDevTransport *tr, uint8_t *d_wire, const uint64_t *d_off,
                                         const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream);

/* ------------------------------------------------ 10. the session table
 *
 * One long-lived transport object (section 9) as a server's table of
 * sessions: its n slots are keyed from finished handshake batches and
 * un-keyed when a connection closes, on the device and in stream order, and a
 * call may address only the slots that have traffic.  Nothing of section 9
 * changes: an object from noise_aead_dev_transport_new behaves byte for byte
 * as described there.
 *
 * Slots and their state.  Each of an object's n slots is keyed or unkeyed,
 * the batch form of noise_cipherstate_has_key: one byte per slot (1 / 0) in a
 * device array the object owns, which _has_key returns (NULL for n == 0 and
 * for a NULL tr).  An object from noise_aead_dev_transport_new starts with
 * every slot keyed; _new_unkeyed makes one with every slot unkeyed, every
 * context byte 0 and every nonce 0.  In any frame call (section 9's or the
 * _of ones) an unkeyed slot gives result = {0, 0, NOISE_ERROR_INVALID_STATE,
 * 0}, what noise_wire_seal / _open / _echo return for an unkeyed state
 * (wire.c:199), checked before anything else as there: none of the slot's
 * stream is read or written, it takes no frame numbers (its count is 0, so it
 * never moves another session's place under the cap), and it reports
 * NOISE_ERROR_INVALID_STATE on either side of a cut too.
 *
 * _set_keys is the batch form of noise_cipherstate_init_key on both states of
 * a slot.  Entry j (j < m) addresses slot d_slots[j]; its keys are the 32
 * bytes at d_k1 + 32 j and d_k2 + 32 j, the packing
 * noise_aead_dev_handshake_split and noise_aead_dev_split write; the role
 * picks send and receive as for _new.  It builds both key contexts of the
 * slot, sets both nonces to 0 (init_key resets n, cipherstate.c:231-233, so a
 * keyed slot is simply re-keyed) and marks the slot keyed.  With d_status
 * given (noise_aead_dev_handshake_status(hs) as it lies; it may be NULL), an
 * entry whose d_status[j] != 0 is cleared instead, as by _clear_keys: a
 * failed handshake never becomes a session and nobody reads a status on the
 * host.  The keys are consumed once `stream` has passed the call.
 *
 * _clear_keys zeroes every byte of both contexts of each named slot, zeroes
 * both nonces and marks the slot unkeyed.
 *
 * Both: a slot number >= n is ignored, nothing is read or written for it.
 * The slot numbers of one call must be distinct; they live in device memory,
 * so that is the caller's guarantee, unchecked like the ragged calls' ranges.
 * Both are asynchronous on `stream`, allocate nothing, copy nothing to the
 * host and never synchronise.  Slots not named are unchanged byte for byte:
 * contexts, nonces and state.
 *
 * _seal_frames_of / _open_frames_of / _echo_frames_of are the three frame
 * calls over a list of slots.  Entry j (j < m) is slot d_slots[j] with its
 * stream the d_len[j] bytes at d_wire + d_off[j], and its result goes to
 * d_result[j]: the per-call arrays are m long, not n long.  Frames are
 * numbered across the call in list order.  max_frames is this call's cap: 0
 * means the object's own, and a value above the object's is refused.  The
 * AEAD launches cover only that many records, so a small tick on a large
 * table does not pay for the table's max_frames.  For each keyed in-range
 * entry the outcome (bytes, result, both nonces) is that of the call of
 * section 9 on a batch made of exactly the listed sessions in list order.  An
 * out-of-range entry (d_slots[j] >= n) gives {0, 0, NOISE_ERROR_INVALID_PARAM,
 * 0} and takes no frame numbers; an unkeyed entry behaves as described above.
 * The listed slots must be distinct: the caller's guarantee.  The three calls
 * of section 9 are the list 0 .. n-1 with max_frames == 0.
 *
 * Checked on the host before any launch, in this order:
 *   - _new_unkeyed: as _new, without the key pointers;
 *   - _set_keys, _clear_keys and the _of calls:
 *       1. a NULL tr gives NOISE_ERROR_INVALID_PARAM;
 *       2. m == 0 gives NOISE_ERROR_NONE, and nothing is launched;
 *       3. m > n gives NOISE_ERROR_INVALID_PARAM;
 *       4. a NULL d_slots, and a NULL d_k1 or d_k2 (_set_keys), d_wire, d_off,
 *          d_len or d_result (_of), give NOISE_ERROR_INVALID_PARAM;
 *       5. _of only: a max_frames above the object's gives
 *          NOISE_ERROR_INVALID_PARAM;
 *       6. _of only: [d_result, + 16 m) meeting [d_off, + 8 m), [d_len, + 4 m)
 *          or [d_slots, + 4 m) gives NOISE_ERROR_INVALID_PARAM.
 *     An _of call whose scan of m items would need more scratch than _new
 *     carved for n gives NOISE_ERROR_SYSTEM (nothing is launched). */
int noise_aead_dev_transport_new_unkeyed(NoiseAeadDevTransport **tr, int cipher_id, int role,
                                         uint32_t n, uint32_t max_frames, void *stream);
int noise_aead_dev_transport_set_keys(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m,
                                      const uint8_t *d_k1, const uint8_t *d_k2,
                                      const uint8_t *d_status /* may be NULL */, void *stream);
int noise_aead_dev_transport_clear_keys(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m,
                                        void *stream);
const uint8_t *noise_aead_dev_transport_has_key(const NoiseAeadDevTransport *tr); /* n bytes, 1 / 0; NULL for n == 0 */
int noise_aead_dev_transport_seal_frames_of(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m,
                                            uint32_t max_frames, uint8_t *d_wire, const uint64_t *d_off,
                                            const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream);
int noise_aead_dev_transport_open_frames_of(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m,
                                            uint32_t max_frames, uint8_t *d_wire, const uint64_t *d_off,
                                            const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream);
int noise_aead_dev_transport_echo_frames_of(NoiseAeadDevTransport *tr, const uint32_t *d_slots, uint32_t m,
                                            uint32_t max_frames, uint8_t *d_wire, const uint64_t *d_off,
                                            const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream);

/* ------------------------------------------------ 11. datagram transport
 *
 * The session table (section 10) for traffic that is lost, duplicated and
 * reordered: the Noise specification's "out-of-order transport messages".
 * The sender puts the 64-bit nonce on the wire, the receiver uses it for that
 * one message, and an anti-replay window per slot, kept on the device, refuses
 * a counter it has accepted before.  The reference has only the primitive,
 * noise_cipherstate_set_nonce (cipherstate.c:518-535), which refuses to go
 * backwards.  Nothing of sections 9 and 10 changes: the stream calls never
 * read or write a window, and the datagram open never reads or writes a
 * receive nonce.
 *
 * Wire format.  A session's bytes lie as in sections 9 and 10: entry j's
 * stream is the d_len[j] bytes at d_wire + d_off[j], frames of a 2-byte
 * big-endian L and L bytes.  In a datagram frame the L bytes are an 8-byte
 * little-endian counter, then CT || tag: L >= 24, and the payload is L - 24
 * bytes.  The walk is that of section 9 with 24 in place of 16: a partial
 * frame ends it with NOISE_ERROR_NONE, a complete frame with L < 24 ends it
 * with NOISE_ERROR_INVALID_LENGTH and is left untouched (a packer knows its
 * datagrams' lengths and packs no runt); frames are numbered across the call
 * in list order and the cap cuts as in section 9; an unkeyed entry gives
 * NOISE_ERROR_INVALID_STATE and an out-of-range one NOISE_ERROR_INVALID_PARAM,
 * with no frames and nothing read or written, as in section 10.  d_slots ==
 * NULL means entry j is slot j; max_frames == 0 means the object's own cap.
 *
 * The replay state of a slot: top, the highest accepted counter + 1 (0 when
 * nothing has been accepted), and a bitmap of 1024 bits; bit c % 1024 stands
 * for counter c.  For a counter c:
 *   - c == 2^64 - 1 is refused: the CipherState never uses that nonce;
 *   - c >= top is fresh.  On acceptance the bits of the counters top .. c - 1
 *     are cleared (the whole bitmap if c - top >= 1024), bit c is set and top
 *     becomes c + 1;
 *   - c < top with top - c > 1024 is refused as too old;
 *   - otherwise c is refused if its bit is set, else it is fresh, and on
 *     acceptance its bit is set.
 * _set_keys and _clear_keys reset a slot's state to all zero, as init_key
 * resets n; an object starts with every window zero.  _replay returns the
 * object's device array of n x {uint64 top; uint64 seen[16]} (136 bytes per
 * slot), which a caller may read or write in stream order, and the window
 * size in *bits (bits may be NULL); NULL for a NULL tr and for n == 0.
 *
 * _seal_datagrams is _seal_frames_of on frames with 8 bytes of room in front:
 * frame k of the entry gets the counter send + k written into those 8 bytes,
 * and its L - 24 plaintext bytes and 16 bytes of room become CT || tag under
 * that counter.  send advances by the frames taken; the walk stops with
 * NOISE_ERROR_INVALID_NONCE where send + k == 2^64 - 1.  Result and cap as in
 * section 10.
 *
 * _open_datagrams judges every walked frame alone; nothing is sticky, and a
 * forged frame costs its session nothing.  d_frame_status[first + k] is the
 * status of the entry's frame k:
 *   0  accepted: the plaintext is in place at body + 8, the tag bytes are left
 *      as they were;
 *   1  the tag failed: the frame is byte for byte untouched;
 *   5  refused by the window (NOISE_ERROR_INVALID_NONCE, what set_nonce
 *      answers for a counter behind the state).
 * Statuses 2 to 4 do not occur.  Bytes of d_frame_status at or past the
 * call's total of walked frames are not written.  The statuses and the window
 * after the call are those of processing the entry's frames one by one in
 * stream order: the window refuses the counter -> 5; else the tag is verified
 * under the receive key with nonce = counter, and a failed tag -> 1; else the
 * counter is accepted -> 0.  A forged frame never moves the window.  In the
 * result, frames, consumed and error are the walk's; accepted counts the
 * entry's frames with status 0; first is the number of its first frame (for
 * an entry after the cut, which has no frames, the number it would have had;
 * 0 for an entry that is not live).
 * A frame with status 5 holds its bytes as given, with one exception: a
 * frame that only an earlier frame of the same call made a replay (a
 * duplicate inside the call, or a counter that a jump of top inside the call
 * left behind) was opened before the window moved, so if its own tag verified
 * it may hold its plaintext (tag bytes as they were) — never anything else
 * and never unauthenticated plaintext.  A frame the window refused as it
 * stood before the call is never touched and costs no AEAD work.
 *
 * Both calls are asynchronous on `stream`, allocate nothing, copy nothing to
 * the host and never synchronise.  The listed slots must be distinct and the
 * streams disjoint: the caller's guarantee.
 *
 * Checked on the host before any launch, in this order:
 *   1. a NULL tr gives NOISE_ERROR_INVALID_PARAM;
 *   2. m == 0 gives NOISE_ERROR_NONE, and nothing is launched;
 *   3. m > n gives NOISE_ERROR_INVALID_PARAM;
 *   4. a NULL d_wire, d_off, d_len or d_result, and for the open a NULL
 *      d_frame_status, give NOISE_ERROR_INVALID_PARAM;
 *   5. a max_frames above the object's gives NOISE_ERROR_INVALID_PARAM;
 *   6. d_result (16 m bytes for the seal, 24 m for the open) meeting
 *      [d_off, + 8 m), [d_len, + 4 m) or a given [d_slots, + 4 m), and for
 *      the open [d_frame_status, + the call's cap) meeting any of those or
 *      d_result, give NOISE_ERROR_INVALID_PARAM.
 * A call whose scan of m items would need more scratch than _new carved for n
 * gives NOISE_ERROR_SYSTEM (nothing is launched). */
typedef struct NoiseAeadDatagramResult {
    uint32_t frames;    /* frames of this entry walked by the call */
    uint32_t consumed;  /* bytes they span, headers included */
    int32_t  error;     /* the walk's stop: NOISE_ERROR_NONE / _INVALID_LENGTH; _INVALID_STATE / _INVALID_PARAM for an entry that is not live */
    uint32_t accepted;  /* frames of this entry whose status is 0 */
    uint64_t first;     /* number of this entry's first frame in d_frame_status */
} NoiseAeadDatagramResult;

int noise_aead_dev_transport_seal_datagrams(NoiseAeadDevTransport *tr, const uint32_t *d_slots /* may be NULL */,
                                            uint32_t m, uint32_t max_frames, uint8_t *d_wire, const uint64_t *d_off,
                                            const uint32_t *d_len, NoiseAeadTransportResult *d_result, void *stream);
int noise_aead_dev_transport_open_datagrams(NoiseAeadDevTransport *tr, const uint32_t *d_slots /* may be NULL */,
                                            uint32_t m, uint32_t max_frames, uint8_t *d_wire, const uint64_t *d_off,
                                            const uint32_t *d_len, NoiseAeadDatagramResult *d_result,
                                            uint8_t *d_frame_status, void *stream);
uint64_t *noise_aead_dev_transport_replay(const NoiseAeadDevTransport *tr, uint32_t *bits);

/* ------------------------------------------------ 12. rekey on the device
 * CipherState.Rekey() of the Noise specification (4.2, 11.3): k = REKEY(k),
 * n untouched, for raw keys and for the slots of a transport object — what a
 * session that lives as long as its server needs, with nothing passing
 * through the host.  The reference (noise-c v0.0.1) has no rekey; this is the
 * specification's, on the reference's nonce layouts.
 *
 * REKEY(k) is the first 32 bytes of ENCRYPT(k, 2^64 - 1, "", 32 zero bytes);
 * no tag is computed:
 *   ChaChaPoly  bytes 0..31 of the ChaCha20 block under k, block counter 1
 *               (counter 0 is the Poly1305 key), 64-bit IV 0xFFFFFFFFFFFFFFFF;
 *   AES-GCM     AES256_k(00000000 || FF x 8 || 00000002) ||
 *               AES256_k(00000000 || FF x 8 || 00000003): the first two CTR
 *               blocks under J0 = 0^32 || BE64(2^64 - 1) || 00000001.
 *
 * noise_aead_dev_rekey: key i is the 32 bytes at d_keys + 32 i, its successor
 * goes to d_out + 32 i (the packing of noise_aead_dev_split and _prepare).  No
 * alignment is needed; d_out == d_keys (in place) is allowed.  Asynchronous on
 * `stream`, allocates nothing, never synchronises.  Checked on the host before
 * any launch, in this order:
 *   1. a cipher other than ChaChaPoly / AESGCM gives NOISE_ERROR_UNKNOWN_ID,
 *      also with n == 0;
 *   2. n == 0 gives NOISE_ERROR_NONE, and nothing is launched;
 *   3. a NULL pointer gives NOISE_ERROR_INVALID_PARAM;
 *   4. [d_out, + 32 n) meeting [d_keys, + 32 n) other than exactly in place
 *      gives NOISE_ERROR_INVALID_PARAM.
 *
 * noise_aead_dev_transport_rekey: entry j (j < m) is slot d_slots[j], or slot
 * j when d_slots is NULL, as in section 11.  The directions it rekeys are
 * directions & (d_which ? d_which[j] : 3): bit 0 is send, bit 1 is receive.
 * The per-entry byte lets a caller's own device-side policy (a kernel that
 * looks at the nonces, say) pick the slots without the host reading anything,
 * as d_status does for _set_keys.  For each chosen direction the slot's key
 * context becomes, byte for byte, the context noise_aead_dev_prepare builds
 * from REKEY(k) of the key it was built from.  Nothing else of the object
 * changes: not the nonce of that direction (the specification's Rekey leaves n
 * alone; _nonces is writable for a caller that wants otherwise), not the
 * anti-replay window, not the state byte, not the other direction, no slot
 * that is not named.  An entry whose slot is out of range or unkeyed is
 * ignored: nothing is read or written, and an unkeyed slot stays all-zero.
 * The listed slots must be distinct: the caller's guarantee, as in section 10.
 * Calls in stream order compose: three calls with no synchronisation between
 * them leave REKEY(REKEY(REKEY(k))).  Both peers of a session rekey the same
 * direction at the same counter: the sender its send direction, the receiver
 * its receive direction.  Asynchronous on
 * `stream`, allocates nothing, copies nothing to the host and never
 * synchronises.  Checked on the host before any launch, in this order:
 *   1. a NULL tr gives NOISE_ERROR_INVALID_PARAM;
 *   2. m == 0 gives NOISE_ERROR_NONE, and nothing is launched;
 *   3. m > n gives NOISE_ERROR_INVALID_PARAM;
 *   4. directions equal to 0 or above 3 gives NOISE_ERROR_INVALID_PARAM.
 * A refused call leaves the object as it was. */
int noise_aead_dev_rekey(int cipher_id, const uint8_t *d_keys, uint32_t n, uint8_t *d_out, void *stream);

#define NOISE_AEAD_REKEY_SEND    1u
#define NOISE_AEAD_REKEY_RECEIVE 2u
int noise_aead_dev_transport_rekey(NoiseAeadDevTransport *tr, const uint32_t *d_slots /* may be NULL */, uint32_t m,
                                   uint32_t directions, const uint8_t *d_which /* may be NULL */, void *stream);

/* ------------------------------------------------ 13. packet transport
 * The datagram calls of section 11 for traffic as a socket delivers it: a
 * receive batch (recvmmsg, a NIC ring) is a list of packets in arrival order,
 * each with its session index, the same session many times and interleaved
 * with others.  Section 11 wants one framed stream per entry and distinct
 * slots, which costs a server a host sort and a gather per tick.  Here a call
 * takes a device list of {off, len, slot} in any order with any repetition,
 * answers with one status byte per packet, and leaves every slot's window and
 * send counter exactly as if the packets had been processed one by one in
 * list order.  Nothing of sections 9 to 12 changes: their bytes, results and
 * memory footprint are what they were, and an object that never reserves is
 * byte for byte the object it was.
 *
 * A packet is a section-11 frame without its 2-byte header (a UDP datagram
 * knows its own length): the len bytes at d_wire + off are an 8-byte
 * little-endian counter, then CT || tag; the payload is len - 24 bytes.
 * Nothing needs alignment.  A packet may point at the body of a frame of a
 * section-11 wire (off the body, len its L), so the same bytes can be opened
 * by either call.  The packets' byte ranges are pairwise disjoint: the
 * caller's guarantee, unchecked, as for the ragged calls.
 *
 * _reserve_packets allocates, once per object, what a packet call needs for
 * up to max_packets packets: sort keys and the order (both double-buffered),
 * descriptors, AEAD statuses and the sort's scratch — about 65 bytes per
 * packet, a device allocation of its own, zeroed on `stream`; what _new
 * allocated is not touched.  _free scrubs and frees it with the rest.  After
 * it a packet call is asynchronous on `stream`, allocates nothing, copies
 * nothing to the host and never synchronises.  Checked in this order:
 *   1. a NULL tr gives NOISE_ERROR_INVALID_PARAM;
 *   2. max_packets == 0 or above 2^31 gives NOISE_ERROR_INVALID_PARAM;
 *   3. an object that has reserved gives NOISE_ERROR_INVALID_STATE;
 *   4. an allocation that fails gives NOISE_ERROR_NO_MEMORY, and the object is
 *      as it was.
 *
 * d_status[p] is the status of packet p; the causes are looked for in this
 * order:
 *   6  no session (NOISE_ERROR_INVALID_STATE's number): slot >= n, or the slot
 *      is unkeyed;
 *   4  len < 24 or len > 65535 (NOISE_ERROR_INVALID_LENGTH's);
 *   5  the counter is refused.  Open: by the slot's window.  Seal: the slot's
 *      send counter has run out, the packet would get 2^64 - 1;
 *   1  open only: the tag failed;
 *   0  done.
 * Of a packet with status 6 or 4 nothing is read or written; it takes no
 * counter, meets no window and moves no other packet's counter.  On an object
 * with n == 0 every packet gets 6.
 *
 * _open_packets: the statuses and every slot's window after the call are
 * those of processing the packets one by one in list order with the rule of
 * section 11: the window refuses the counter -> 5; else the tag is verified
 * under the receive key with nonce = counter, and a failed tag -> 1; else the
 * counter is accepted -> 0, the plaintext is in place at off + 8 and the tag
 * bytes are left as they were.  A forged packet never moves a window and is
 * byte for byte untouched.  The receive nonce is neither read nor written.  A
 * packet the window refuses as it stood before the call costs no AEAD work
 * and is never touched.  The one exception to "as given" is section 11's: a
 * status-5 packet that only an earlier packet of the same call made a replay
 * (a duplicate at another offset, or a counter that a jump of top inside the
 * call left behind) may hold its plaintext if its own tag verified — never
 * anything else and never unauthenticated plaintext.
 *
 * _seal_packets: packet p is 8 bytes of room, len - 24 bytes of plaintext and
 * 16 bytes of room.  Among the packets of its slot that are sealed, in list
 * order, the k-th gets the counter send + k written in front and its body
 * becomes CT || tag under that counter; send advances by the packets sealed.
 * Where send + k would be 2^64 - 1, that packet and every later packet of the
 * slot in the call get status 5 and are untouched; send stays at 2^64 - 1.
 *
 * Both calls share send and the windows with the calls of section 11 and with
 * _set_keys, _clear_keys, _rekey, _replay and _nonces; calls of all kinds
 * compose in stream order.
 *
 * Checked on the host before any launch, in this order:
 *   1. a NULL tr gives NOISE_ERROR_INVALID_PARAM;
 *   2. count == 0 gives NOISE_ERROR_NONE, and nothing is launched, reserved or
 *      not;
 *   3. an object that has not reserved gives NOISE_ERROR_INVALID_STATE;
 *   4. count > max_packets gives NOISE_ERROR_INVALID_PARAM;
 *   5. a NULL d_packets, d_wire or d_status gives NOISE_ERROR_INVALID_PARAM;
 *   6. [d_status, + count) meeting [d_packets, + 16 count) gives
 *      NOISE_ERROR_INVALID_PARAM.
 * A refused call leaves the object as it was.  A call whose sort of count
 * items would need more scratch than was reserved gives NOISE_ERROR_SYSTEM
 * (nothing is launched). */
typedef struct NoiseAeadPacket {
    uint64_t off;   /* the packet's bytes start at d_wire + off; nothing needs alignment */
    uint32_t len;   /* 8-byte little-endian counter, then CT || tag: 24 .. 65535 */
    uint32_t slot;  /* its slot of the table; slots repeat and come in any order */
} NoiseAeadPacket;  /* 16 bytes */

int noise_aead_dev_transport_reserve_packets(NoiseAeadDevTransport *tr, uint32_t max_packets, void *stream);
int noise_aead_dev_transport_seal_packets(NoiseAeadDevTransport *tr, const NoiseAeadPacket *d_packets, uint32_t count,
                                          uint8_t *d_wire, uint8_t *d_status, void *stream);
int noise_aead_dev_transport_open_packets(NoiseAeadDevTransport *tr, const NoiseAeadPacket *d_packets, uint32_t count,
                                          uint8_t *d_wire, uint8_t *d_status, void *stream);

/* ------------------------------------------------ 14. packet echo
 * The third verb of the packet calls, as _echo_frames is of the stream calls:
 * the reference echo server's tick (echo-server.c: read, decrypt, encrypt,
 * write) over a receive batch of section 13.  A UDP server that answers what
 * it accepts otherwise calls _open_packets, needs the list of the accepted
 * packets (a read of d_status on the host in the middle of its tick, or a
 * kernel of its own), and calls _seal_packets, which classifies and sorts
 * again.  Here one call opens the list and seals the replies in place, so that
 * handshake -> _set_keys -> echo ticks runs with the host reading nothing.
 *
 * Definition.  The bytes, the statuses, every slot's window and every slot's
 * send counter after the call are those of two calls in sequence:
 *   1. _open_packets over the list;
 *   2. _seal_packets over the sub-list of the packets that step 1 gave status
 *      0, in list order, on the same bytes.
 * d_status[p] is the open's status if that is not 0, else the seal's.  The
 * causes are therefore looked for in section 13's order:
 *   6  no session;
 *   4  len < 24 or len > 65535;
 *   5  refused by the slot's window;
 *   1  the tag failed;
 *   5  the slot's send counter has run out;
 *   0  echoed.
 * A packet echoed with status 0 keeps its len and its place: the 8 bytes in
 * front hold the send counter it got, send + k for the k-th echoed packet of
 * its slot in list order; the len - 24 bytes behind them are its payload
 * sealed under the slot's send key and that counter, and the tag follows.  The
 * counter it arrived with is gone.  Of a packet with status 6 or 4 nothing is
 * read or written.  A packet with status 1 is byte for byte untouched.  A
 * packet the window refuses is never read or written, with section 11's one
 * exception: a packet that only an earlier packet of the same call made a
 * replay may hold its plaintext.  None of these takes a send counter, and none
 * moves another packet's.
 *
 * Where send + k would be 2^64 - 1, that packet and every later accepted
 * packet of the slot in the call get status 5.  They were opened: the window
 * has accepted their counters, and their bytes are what _open_packets leaves
 * for an accepted packet — the received counter, the plaintext, the tag bytes
 * as they were.  send stays at 2^64 - 1.
 *
 * The receive nonce is neither read nor written.  The call shares send and the
 * windows with the calls of sections 11 to 13 and with _set_keys, _clear_keys,
 * _rekey, _replay and _nonces, and composes with them in stream order.  It
 * uses the reservation of _reserve_packets and nothing more: the reservation
 * does not grow, and the object's footprint is what it was.  The call is
 * asynchronous on `stream`, allocates nothing, copies nothing to the host and
 * never synchronises.  Nothing of sections 9 to 13 changes in bytes, results
 * or footprint.
 *
 * A packet may point at the body of a frame of a section-11 wire, as in
 * section 13, so framed datagrams are served by this call too; there is no
 * framed form of it (a framed reply stream with holes where packets were
 * refused has no counterpart on the sender's side).
 *
 * Checked on the host before any launch: the six checks of section 13's
 * calls, in that order.  A refused call leaves the object as it was;
 * count == 0 gives NOISE_ERROR_NONE, reserved or not.  A call whose sort would
 * need more scratch than was reserved gives NOISE_ERROR_SYSTEM (nothing is
 * launched). */
int noise_aead_dev_transport_echo_packets(NoiseAeadDevTransport *tr, const NoiseAeadPacket *d_packets, uint32_t count,
                                          uint8_t *d_wire, uint8_t *d_status, void *stream);

/* ------------------------------------------------ 15. Noise Pipes fallback
 * What noise_handshakestate_fallback and the noise_handshakestate_start after
 * it (src/protocol/handshakestate.c:888-1079, :800-885) do for one session,
 * done for some sessions of a batch of section 8: a responder whose static
 * key rotated cannot decrypt the IK first message of a client that cached the
 * old one, and both ends go on with XXfallback, reusing the initiator's
 * ephemeral, without the host reading a status.  By name XXfallback stays out
 * of reach (section 8: NOISE_ERROR_NOT_APPLICABLE); it is reached here, as a
 * call on a running handshake.
 *
 * _fallback makes a second object *fb over the same n session indices.  Its
 * protocol is hs's name with the pattern field replaced by XXfallback, its
 * role the opposite of hs's, its tokens the reference's (patterns.c:444-471):
 * pre-message <- e, then -> e, ee, s, se, then <- s, es.  The former responder
 * is fb's initiator (_get_action: NOISE_ACTION_WRITE_MESSAGE): it keeps the
 * ephemeral it received and its static key pair, forgets the remote static
 * key and takes a fresh ephemeral from cfg.  The former initiator is fb's
 * responder (NOISE_ACTION_READ_MESSAGE): it keeps its ephemeral and its static
 * key pair and forgets both remote keys.  fb copies the public values it
 * keeps into device memory of its own, so hs may be freed first; the
 * private-key pointers (those given to hs's _new, and
 * cfg->d_local_ephemeral_priv) are the caller's and must stay valid and
 * unchanged until fb's split.  Start-up is section 8's with the new name (at
 * most 44 characters), cfg's prologue (the fallback's own: it may differ from
 * hs's in bytes and length) and cfg's PSK (needed again under NoisePSK: _new
 * consumed it), then the pre-message: MixHash of the former initiator's
 * ephemeral public key and, under NoisePSK, MixKey of it (:854-857,
 * :870-873), which sets a key before the first message.  After that every
 * call of section 8 works on fb unchanged: the overheads are 96 and 64.
 *
 * Which sessions take part is decided on the device, per session, from its
 * status in hs.  Session i is eligible when that status is 0 or 1 for a
 * former responder (1: the first message failed; 0: it verified and the
 * responder falls back anyway, :1001-1005) or 0 for a former initiator; a
 * session of status 3 or 4 never received or kept a usable e.  It takes part
 * iff it is eligible, d_select is NULL or d_select[i] != 0, and — with
 * NOISE_AEAD_FALLBACK_ONLY_FAILED — its status in hs is 1.  A session that
 * does not take part has the status 5 in fb, "not in this object": it is
 * inert from the start, as any failed session is (section 8), and fb's split
 * writes zeros for it.  A session that takes part with status 0 gets status 5
 * in hs, so that no session is live in both objects; a status-1 session of hs
 * stays 1.  hs goes on as before for the sessions it keeps.
 *
 * Checked on the host before any launch, in this order:
 *   - hs, cfg or fb NULL: NOISE_ERROR_INVALID_PARAM;
 *   - hs's pattern is not NK, XK, KK or IK (interactive, the responder's
 *     static key known beforehand), or hs is itself a fallback:
 *     NOISE_ERROR_NOT_APPLICABLE;
 *   - anything but exactly one message done — an initiator waiting to read
 *     the second, a responder about to write it: NOISE_ERROR_INVALID_STATE;
 *   - hs was made without a static private key (the NK initiator), or a
 *     former responder's cfg has no d_local_ephemeral_priv:
 *     NOISE_ERROR_LOCAL_KEY_REQUIRED;
 *   - NoisePSK without d_psk: NOISE_ERROR_PSK_REQUIRED;
 *   - prologue_len without d_prologue, a stride other than 0 below the length
 *     (prologue) or below 32 (the keys that are read), a flag other than
 *     NOISE_AEAD_FALLBACK_ONLY_FAILED: NOISE_ERROR_INVALID_PARAM.
 * A refused call leaves hs as it was and *fb NULL.  n == 0 gives a valid fb
 * and launches nothing.  The call is asynchronous on `stream`, copies nothing
 * to the host and never synchronises; a former initiator's cfg needs no key.
 *
 * _fallback_merge folds the two objects' splits into one set of keys for
 * noise_aead_dev_transport_set_keys (section 10), which clears a slot whose
 * status byte is not 0 and wants every session's keys in one orientation.
 * d_k1, d_k2 and the optional d_h hold hs's split as it lies, d_fb_k1,
 * d_fb_k2 and d_fb_h fb's (d_h and d_fb_h: both or neither), d_hs_status is
 * hs's status array.  For session i, by its status in fb:
 *   0     d_k1[i] = d_fb_k2[i], d_k2[i] = d_fb_k1[i], d_h[i] = d_fb_h[i],
 *         d_status[i] = 0: the keys in the original role's orientation, so
 *         the side that sent under k2 still does;
 *   5     nothing of the keys or the hash is written, d_status[i] =
 *         d_hs_status[i];
 *   else  zeros for both keys and the hash, d_status[i] = fb's status.
 * Checked on the host before any launch: a NULL pointer (other than d_h and
 * d_fb_h together) gives NOISE_ERROR_INVALID_PARAM; fb not _COMPLETE
 * NOISE_ERROR_INVALID_STATE; n == 0 NOISE_ERROR_NONE and no launch; an output
 * (d_k1, d_k2, d_h, d_status) that meets an array the call reads (d_fb_k1,
 * d_fb_k2, d_fb_h, d_hs_status, fb's statuses) NOISE_ERROR_INVALID_PARAM.
 * Asynchronous on `stream`. */
#define NOISE_AEAD_FALLBACK_ONLY_FAILED 1u
typedef struct NoiseAeadHandshakeFallbackConfig {
    const uint8_t *d_prologue;  uint64_t prologue_stride; uint32_t prologue_len; /* the fallback's own */
    const uint8_t *d_psk;       uint64_t psk_stride;       /* NoisePSK: needed again, _new consumed it */
    const uint8_t *d_local_ephemeral_priv; uint64_t local_ephemeral_stride; /* the former responder's fresh e */
    const uint8_t *d_select;    /* n bytes, or NULL: every eligible session */
    uint32_t flags;
} NoiseAeadHandshakeFallbackConfig;
int noise_aead_dev_handshake_fallback(NoiseAeadDevHandshake *hs, const NoiseAeadHandshakeFallbackConfig *cfg,
                                      NoiseAeadDevHandshake **fb, void *stream);
int noise_aead_dev_handshake_fallback_merge(const NoiseAeadDevHandshake *fb, const uint8_t *d_hs_status,
                                            uint8_t *d_k1, uint8_t *d_k2, const uint8_t *d_fb_k1,
                                            const uint8_t *d_fb_k2, uint8_t *d_h, const uint8_t *d_fb_h,
                                            uint8_t *d_status, void *stream);

/* ------------------------------------------------ 16. sessions that change their object
 *
 * An object of section 8 runs its n sessions in lockstep: the action, the
 * message index, "is a key set" and the nonce are host values of the whole
 * object, and every message call advances them for the batch.  That fits a
 * two-message pattern.  The third message of XX, XK and XN, and the second of
 * an XXfallback object (section 15), comes back from each client in its own
 * time.  Lockstep stays; what these calls add is that a session can change its
 * object.  A lane of status 5, "not in this object" (section 15), is inert in
 * every call: that is an empty lane.
 *
 * _new_like makes an empty object of `capacity` lanes at the position of
 * `like`: its protocol name, fallback flag, role, action, message index, "is
 * a key set", nonce, hash length and cipher context size.  Every lane has the
 * status 5 and every other device byte the object owns is zero.  Each of
 * like's two private keys (static, ephemeral) on its own: a key like holds per
 * session (stride != 0) gets capacity x 32 bytes the object owns, read at
 * stride 32 from then on; a key like holds once for all (stride 0) is read
 * through like's pointer, which stays the caller's and must stay valid, and
 * its one public-key row is copied now; a key like never had stays absent.
 * After that the object is an ordinary one: every call of sections 8 and 15
 * but _fallback serves it, over all `capacity` lanes, and _free scrubs the
 * owned rows with the rest.  Checked on the host, in this order: a NULL out or
 * like gives NOISE_ERROR_INVALID_PARAM; like at NOISE_ACTION_COMPLETE or
 * _NONE gives NOISE_ERROR_INVALID_STATE.  capacity == 0 gives a valid object
 * that allocates and launches nothing.  *out is NULL after a refused call.
 *
 * _move: entry j (j < m) moves the session in lane d_src_lanes[j] of src into
 * lane d_dst_lanes[j] of dst.  Either list may be NULL and then means
 * 0 .. m-1.  d_result may be NULL; otherwise byte j receives the outcome,
 * the causes tested in this order:
 *   NOISE_AEAD_MOVE_RANGE  3  a lane number >= n of its object; nothing is
 *                             read or written for the entry;
 *   NOISE_AEAD_MOVE_EMPTY  1  the source lane has the status 5;
 *   NOISE_AEAD_MOVE_TAKEN  2  the destination lane has another status than 5;
 *   NOISE_AEAD_MOVED       0  otherwise.
 * A failed session (status 1, 3 or 4) moves with its status, so that the
 * status array of the object it ends in still clears its slot in _set_keys
 * (section 10).  A moved entry copies ck, h, k, the status, the remote
 * ephemeral and static keys, the public-key rows held per session and the
 * private-key rows held per session — read from src's pointer and stride, the
 * caller's memory or owned rows, no alignment assumed — into dst's owned rows.
 * Then the source lane is scrubbed: every one of those rows that src owns is
 * zeroed, with the lane's AES-GCM context, and its status set to 5.  The
 * caller's own key memory is never written.  AES-GCM contexts are not copied:
 * a dst with a key set prepares them from k before its next AEAD step, as
 * after a MixKey.  The lanes of one call must be distinct per object; they
 * live in device memory, so that is the caller's guarantee, unchecked as for
 * _set_keys.
 *
 * Checked on the host before any launch, in this order; a refused call leaves
 * both objects as they were:
 *   1. a NULL object gives NOISE_ERROR_INVALID_PARAM;
 *   2. src == dst gives NOISE_ERROR_INVALID_PARAM;
 *   3. the two objects must be at the same position — name, fallback flag,
 *      role, action, message index, "is a key set" and nonce all equal — and
 *      the action NOISE_ACTION_WRITE_MESSAGE, _READ_MESSAGE or _SPLIT:
 *      otherwise NOISE_ERROR_INVALID_STATE;
 *   4. for each private key, both objects hold it per session and dst in rows
 *      it owns (dst came from _new_like), or both hold it once for all through
 *      the same pointer, or neither holds it: otherwise
 *      NOISE_ERROR_INVALID_PARAM;
 *   5. m == 0 gives NOISE_ERROR_NONE, and nothing is launched;
 *   6. a NULL list with m above that object's n gives
 *      NOISE_ERROR_INVALID_PARAM;
 *   7. [d_result, + m) meeting [d_dst_lanes, + 4 m) or [d_src_lanes, + 4 m)
 *      gives NOISE_ERROR_INVALID_PARAM.
 *
 * _drop is the scrub half alone, for sessions that timed out: the rows of the
 * named lanes are zeroed and their status set to 5.  A lane >= n is ignored.
 * An object from _new may drop as well (its caller's key memory is not
 * written).  Checked as _clear_keys (section 10): a NULL hs gives
 * NOISE_ERROR_INVALID_PARAM; m == 0 NOISE_ERROR_NONE and no launch; m > n or a
 * NULL d_lanes NOISE_ERROR_INVALID_PARAM.  The lanes must be distinct.
 *
 * All three are asynchronous on `stream`, copy nothing to the host and never
 * synchronise; _move and _drop allocate nothing.
 *
 * What stays out.  _fallback from an object made by _new_like gives
 * NOISE_ERROR_NOT_APPLICABLE: the fallback would read ephemeral rows owned by
 * an object that may be freed first.  _fallback_merge pairs the lanes of two
 * objects by index and knows nothing of moves: a cohort taken out of a
 * fallback object does not merge, it hands its own split to _set_keys with
 * the two key pointers exchanged (d_k1 = the split's k2, d_k2 = its k1), which
 * is the orientation of the original role.  There is no compaction by a
 * device-side predicate, no move between positions and no growing of an
 * object.
 *
 * The flow: cohorts of first messages are read and answered in objects of
 * their own; each cohort is moved whole into one long-lived pool object made
 * by _new_like; each tick the host lists the pool lanes whose last message
 * arrived, as it lists the transport's slots, makes _new_like(pool, m), moves
 * those lanes into it, reads, splits, calls _set_keys with the slot list and
 * the cohort's status array, and frees the cohort. */
#define NOISE_AEAD_MOVED      0
#define NOISE_AEAD_MOVE_EMPTY 1
#define NOISE_AEAD_MOVE_TAKEN 2
#define NOISE_AEAD_MOVE_RANGE 3
int noise_aead_dev_handshake_new_like(NoiseAeadDevHandshake **out, const NoiseAeadDevHandshake *like,
                                      uint32_t capacity, void *stream);
int noise_aead_dev_handshake_move(NoiseAeadDevHandshake *dst, const uint32_t *d_dst_lanes /* may be NULL */,
                                  NoiseAeadDevHandshake *src, const uint32_t *d_src_lanes /* may be NULL */,
                                  uint32_t m, uint8_t *d_result /* may be NULL */, void *stream);
int noise_aead_dev_handshake_drop(NoiseAeadDevHandshake *hs, const uint32_t *d_lanes, uint32_t m, void *stream);

/* ------------------------------------------------ 17. batched Ed25519
 *
 * n calls of noise_signstate_verify, or of noise_signstate_sign, for Ed25519
 * (src/protocol/signstate.c:544-597 over src/backend/ref/sign-ed25519.c and
 * src/crypto/ed25519/ed25519.c:45-116) in one launch, so that a responder
 * that learns a client's static key in a handshake message can decide whether
 * a certificate authorises it, and hand the verdict to
 * noise_aead_dev_transport_set_keys (section 10), without a host round trip.
 * The three calls are stateless, as section 7's are: there is no object, the
 * keys are the caller's arrays.  Entry i takes the 32-byte key at ptr +
 * i*stride; a key stride of 0 is one key for all n entries (one certificate
 * authority verifying n certificates), any other key stride must be at least
 * 32.  Message i is the d_msg_len[i] bytes at d_msg + d_msg_off[i]: ragged, as
 * the _ragged calls of section 8 take their messages, in any order, and two
 * entries may share a message.  No pointer, stride or offset needs any
 * alignment.
 *
 * noise_aead_dev_sign_verify.  Entry i is exactly ed25519_sign_open
 * (ed25519.c:93-116) on message i, the public key at d_pub + i*pub_stride and
 * the 64-byte signature R || S at d_sig + i*sig_stride (a stride of at least
 * 64; 0 only with n == 1), the reference's leniencies included:
 *   - a signature with any of the top three bits of S set (sig[63] & 0xE0) is
 *     refused; S is otherwise reduced mod L, not range-checked, so S + L is
 *     accepted where S is (a caller who needs strict signatures checks S < L);
 *   - the public key is decoded as ge25519_unpack_negative_vartime decodes it
 *     (ed25519-donna-impl-base.h:192-239): y is the low 255 bits whatever
 *     their value (2^255 - 19 + k stands for k), the sign bit is not looked
 *     at when x = 0, and a y for which x^2 has no root is refused;
 *   - the check is the comparison of the 32 bytes encode([S]B - [h]A),
 *     h = SHA-512(R || A || M) mod L, with the 32 bytes of R.  R is never
 *     decoded, so a non-canonical R is refused; nothing is multiplied by the
 *     cofactor, so keys of small order verify what the equation says they do.
 * d_status[i] is 0 where the reference returns NOISE_ERROR_NONE and 6 where it
 * returns NOISE_ERROR_INVALID_SIGNATURE (section 8's status space).  With
 * d_status_in (typically noise_aead_dev_handshake_status(hs)), an entry whose
 * input status is non-zero does no work and reads nothing of its own — not its
 * offset, its length, its key nor its signature — and d_status[i] =
 * d_status_in[i]; the output array is then directly the d_status of
 * noise_aead_dev_transport_set_keys.  d_status == d_status_in is allowed: the
 * merge happens in place.  Everything verify reads is public, and its running
 * time depends on it.
 *
 * noise_aead_dev_sign_public is ed25519_publickey (ed25519.c:45-55) of the
 * 32-byte seed at d_priv + i*priv_stride: the private key of a NoiseSignState
 * is that seed.  Public key i goes to d_pub_out + 32*i.
 * noise_aead_dev_sign is ed25519_sign (ed25519.c:58-91) of message i with
 * seed i and the public key at d_pub + i*pub_stride, which is taken as given
 * and never re-derived, as noise_signstate_sign signs with the stored key.
 * Signature i goes to d_sig_out + 64*i.  Signing is deterministic: the bytes
 * are the reference's.  There is no key generation: a seed is 32 bytes of the
 * caller's entropy, as an ephemeral private key is.
 *
 * Constant time, for _sign_public and _sign: [k]B is 253 doublings with an
 * addition at every step whose operand is the identity or B by mask; the
 * scalars mod L are reduced without a branch; no branch, address, table index
 * or loop bound depends on a bit of the seed, of the secret scalar, of the
 * prefix, of r or of an intermediate value.  The seed's hash and the r hash
 * run through the byte buffer of the device's SHA-512, indexed by position
 * only, as the handshake kernels' keys are; the curve arithmetic of all three
 * calls keeps its points in registers.  The message lengths are public.
 *
 * Checked on the host before any launch, in this order: sign_id other than
 * NOISE_SIGN_ED25519 gives NOISE_ERROR_UNKNOWN_ID; n == 0 gives
 * NOISE_ERROR_NONE and touches nothing; otherwise NOISE_ERROR_INVALID_PARAM
 * for a NULL pointer (d_status_in alone may be NULL), for a key stride in
 * 1..31, for a signature stride in 1..63 or of 0 with n > 1, and for an output
 * range ([d_status, + n), [d_pub_out, + 32 n), [d_sig_out, + 64 n)) that meets
 * an input key span ([ptr, + (n - 1)*stride + 32)), the signature span
 * ([d_sig, + (n - 1)*sig_stride + 64)), the offset array [d_msg_off, + 8 n),
 * the length array [d_msg_len, + 4 n) or [d_status_in, + n) — the one
 * exception being d_status == d_status_in exactly.  The message spans are the
 * caller's guarantee, as for every ragged call.  A refused call writes
 * nothing.  Device pointers, asynchronous on `stream`; nothing is allocated
 * and nothing synchronises.
 *
 * What stays out: the batch equation (ed25519_sign_open_batch), a host
 * NoiseSignState object, keypair generation, and any parsing of a
 * certificate: the caller says where the signed bytes and the signature lie. */
int noise_aead_dev_sign_verify(int sign_id, const uint8_t *d_pub, uint64_t pub_stride,
                               const uint8_t *d_sig, uint64_t sig_stride,
                               const uint8_t *d_msg, const uint64_t *d_msg_off, const uint32_t *d_msg_len,
                               uint32_t n, const uint8_t *d_status_in /* may be NULL */, uint8_t *d_status,
                               void *stream);
int noise_aead_dev_sign_public(int sign_id, const uint8_t *d_priv, uint64_t priv_stride, uint32_t n,
                               uint8_t *d_pub_out, void *stream);
int noise_aead_dev_sign(int sign_id, const uint8_t *d_priv, uint64_t priv_stride,
                        const uint8_t *d_pub, uint64_t pub_stride,
                        const uint8_t *d_msg, const uint64_t *d_msg_off, const uint32_t *d_msg_len,
                        uint32_t n, uint8_t *d_sig_out, void *stream);

/* ------------------------------------------------ error reports
 * include/noise/protocol/errors.h; src/protocol/errors.c:92-127. */
void noise_perror(const char *s, int err);
int noise_strerror(int err, char *buf, size_t size);

/* ------------------------------------------------ test / debug hooks
 * Not part of the reference surface; used by the test suite.
 * noise_aead_debug_batch_stats: GPU rounds and records dispatched by this
 *   thread's last noise_cipherstate_decrypt_batch call (a run of forged
 *   records must cost rounds, not re-dispatches of the whole batch).
 * noise_aead_debug_last_freed_ctx: with NOISE_AEAD_DEBUG_KEEP_FREED=1 in the
 *   environment, freeing a CipherState scrubs its device key context but keeps
 *   the allocation; this returns it (and its size) so a test can read back
 *   zeros.  Leaks by design; never set it in production. */
void noise_aead_debug_batch_stats(uint64_t *rounds, uint64_t *dispatched);
/* noise_aead_debug_worker_stamps: the phase times (10-ns ticks) of the
 *   resident single-record worker's last request on the current device:
 *   fence, inputs in LDS, computed, results written, released (n <= 5). */
void noise_aead_debug_worker_stamps(uint32_t *out, int n);
/* noise_aead_debug_worker_clock_mhz: the shader clock of that request's
 *   compute phase (s_memtime cycles / s_memrealtime time), 0 if none. */
double noise_aead_debug_worker_clock_mhz(void);
/* noise_aead_debug_worker_fast_stamps: shader-cycle stamps through the
 *   worker's latency-first ChaChaPoly path, or its AES-GCM record (n <= 8). */
void noise_aead_debug_worker_fast_stamps(uint32_t *out, int n);
/* noise_aead_debug_worker_placement: where the current device's worker
 *   takes requests: 0 not started, 1 pinned host memory, 2 device memory
 *   written through the BAR (large-BAR devices, NOISE_AEAD_WORKER_VRAM). */
int noise_aead_debug_worker_placement(void);
/* noise_aead_debug_worker_host_ns: the calling thread's last worker call on
 *   the host, ns from its start: packed, doorbell, done seen, returned. */
void noise_aead_debug_worker_host_ns(uint64_t *out, int n);
void *noise_aead_debug_last_freed_ctx(size_t *bytes);
/* noise_aead_debug_workers_resident: request slots (one workgroup each) of
 *   the current device whose worker group is still running (-1: no device). */
int noise_aead_debug_workers_resident(void);
/* noise_aead_debug_worker_launches: worker group kernels launched on the
 *   current device so far. */
unsigned noise_aead_debug_worker_launches(void);
/* noise_aead_debug_worker_group_launches: out[g] = launches of group g
 *   (g < 8), out[8..11] = the relaunch checks by cause (not launched,
 *   slot exiting at the call, slot exiting while waiting, no launch needed). */
void noise_aead_debug_worker_group_launches(unsigned *out, int n);
/* noise_aead_debug_worker_leave_reason / _leave_info: why slot `slot` of
 *   group `group` last left (1 stop, 2 another slot closed the group, 4 idle,
 *   8 lifetime) and its born / leave times (10-ns ticks), lifetime, launch. */
unsigned noise_aead_debug_worker_leave_reason(int group, int slot);
void noise_aead_debug_worker_leave_info(int group, int slot, unsigned *out);
/* noise_aead_debug_last_plan: the printed form of the last batch kernel the
 *   calling thread launched through a noise_aead_dev_* entry point, as
 *   "kernel<template arguments> grid=.. block=.. ..." (dispatch.h plan_print);
 *   "none ..." before the first.  Returns the length it has (snprintf's). */
int noise_aead_debug_last_plan(char *buf, size_t n);
/* noise_aead_debug_f25_op: one operation of the X25519 field arithmetic
 *   (csrc/fe25519.h) on each of n elements, one lane each, so that a test can
 *   put a single carry chain of the device build on its rare paths.  Element
 *   i is the 32 little-endian bytes at d_a + 32*i (and d_b + 32*i for add,
 *   sub and mul; d_b may be NULL for the others); any 256-bit value is an
 *   operand.  The result at d_out + 32*i is the operation's raw output: some
 *   256-bit value congruent to the answer mod 2^255 - 19, canonical only for
 *   FREEZE.  INVERT gives 0 for an operand that is 0 mod 2^255 - 19.
 *   An op outside the list gives NOISE_ERROR_UNKNOWN_ID; n == 0 gives
 *   NOISE_ERROR_NONE and no launch; a NULL pointer, or a d_out range that
 *   meets an operand range, gives NOISE_ERROR_INVALID_PARAM.
 *   Device pointers, asynchronous on `stream`. */
#define NOISE_AEAD_F25_ADD        0
#define NOISE_AEAD_F25_SUB        1
#define NOISE_AEAD_F25_MUL        2
#define NOISE_AEAD_F25_SQ         3
#define NOISE_AEAD_F25_MUL_121665 4
#define NOISE_AEAD_F25_MUL_9      5
#define NOISE_AEAD_F25_FREEZE     6
#define NOISE_AEAD_F25_INVERT     7
int noise_aead_debug_f25_op(int op, const uint8_t *d_a, const uint8_t *d_b, uint32_t n,
                            uint8_t *d_out, void *stream);
/* noise_aead_debug_transport_ctx: a transport object's device array of n key
 *   contexts of one direction (0 send, 1 receive) and, in *ctx_bytes, the
 *   bytes per context (noise_aead_dev_ctx_bytes of its cipher), so that a test
 *   can read back what _set_keys built and _clear_keys zeroed (section 10).
 *   NULL for any other direction, a NULL tr or n == 0. */
const uint8_t *noise_aead_debug_transport_ctx(const NoiseAeadDevTransport *tr, int direction, size_t *ctx_bytes);

/* Default lanes per record the library picks for a standalone uniform seal
 * or open of n records (noise_aead_dev_{seal,open}_uniform, lanes 0) in a
 * FAST layout: ChaChaPoly 1 from 128 Ki records (the one-lane kernels at
 * two waves per SIMD), else 4 or 8, and up to 64 for batches of at most 512
 * records (a VERIFY_FIRST open of at least 64 Ki records: 1); AES-GCM 4.
 * Other layouts and ragged batches keep the multi-lane rules. */
int noise_aead_dev_default_lanes(int cipher_id, uint32_t n_records);
/* ...and for each job of a noise_aead_dev_duplex_uniform launch: ChaChaPoly
 * jobs of at least 64 Ki records in FAST layouts (16-B aligned slots
 * readable up to roundup64(len)) take one lane per record (the LDS-staged
 * one-lane kernels, a seal and an open wave on every SIMD), else as above. */
int noise_aead_dev_duplex_lanes(int cipher_id, uint32_t n_records);

/* Deterministic synthetic bytes (bench/test input): 64-bit LE word w of the
 * output = SplitMix64(seed + word0 + w), SURVEY.md §8d. */
int noise_aead_dev_fill_splitmix(uint8_t *d_out, uint64_t nbytes, uint64_t seed,
                                 uint64_t word0, void *stream);

#ifdef __cplusplus
}
#endif
#endif
