/*
 * launch_dh.hip — batched X25519: noise_aead_dev_dh_calculate and
 * noise_aead_dev_dh_public (include/noise_aead_hip.h section 7).  A
 * translation unit of its own, so the build stays parallel and the
 * no-scratch check of tests/test_dh_host.py compiles in seconds.
 *
 * One lane per session, 64-lane workgroups; all arithmetic is fe25519.h
 * (eight 32-bit limbs in registers, 255 ladder steps, the inversion chain,
 * the freeze).  The host checks (dispatch.h check_dh) run before any launch.
 */
#include "launch.h"

#include "fe25519.h"

using namespace na;

namespace {

constexpr uint32_t DH_BLOCK = 64;

struct DhArgs {
    const uint8_t *priv, *pub;
    uint8_t *out;
    uint64_t priv_stride, pub_stride;
    uint32_t n;
};

/* BASE: the public key of each private key (u = 9, a.pub unused) */
template <bool BASE>
__global__ void __launch_bounds__(DH_BLOCK) x25519_batch(DhArgs a)
{
    const uint32_t i = blockIdx.x * DH_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const F25 k = f25_load(a.priv + (uint64_t)i * a.priv_stride);
    const F25 u = BASE ? f25_small(9) : f25_load(a.pub + (uint64_t)i * a.pub_stride);
    f25_store(a.out + (uint64_t)i * 32, x25519<BASE>(k, u));
}

int run_dh(int dh_id, const uint8_t *d_priv, uint64_t priv_stride, bool has_pub, const uint8_t *d_pub,
           uint64_t pub_stride, uint32_t n, uint8_t *d_out, void *stream)
{
    const int rc = check_dh(dh_id, d_priv, priv_stride, has_pub, d_pub, pub_stride, n, d_out);
    if (rc || !n) return rc;
    const DhArgs a = {d_priv, d_pub, d_out, priv_stride, pub_stride, n};
    return launch_items(has_pub ? x25519_batch<false> : x25519_batch<true>, n, DH_BLOCK, (hipStream_t)stream, a);
}

} // namespace

extern "C" {

int noise_aead_dev_dh_calculate(int dh_id, const uint8_t *d_priv, uint64_t priv_stride,
                                const uint8_t *d_pub, uint64_t pub_stride, uint32_t n,
                                uint8_t *d_shared, void *stream)
{
    return run_dh(dh_id, d_priv, priv_stride, true, d_pub, pub_stride, n, d_shared, stream);
}

int noise_aead_dev_dh_public(int dh_id, const uint8_t *d_priv, uint64_t priv_stride, uint32_t n,
                             uint8_t *d_pub_out, void *stream)
{
    return run_dh(dh_id, d_priv, priv_stride, false, nullptr, 0, n, d_pub_out, stream);
}

} // extern "C"
