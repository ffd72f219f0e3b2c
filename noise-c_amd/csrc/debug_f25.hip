/*
 * debug_f25.hip — noise_aead_debug_f25_op (include/noise_aead_hip.h, test /
 * debug hooks): one field operation of fe25519.h per lane, so that the tests
 * can drive the device forms of the carry chains (__builtin_addc /
 * __builtin_subc) to their rare paths one operation at a time
 * (tests/f25_cases.py, tests/test_gpu_f25.py).  A translation unit of its
 * own: launch_dh.hip keeps exactly its two kernels.
 *
 * One lane per element, 64-lane workgroups; the operation is the same for the
 * whole launch, so the switch is a uniform branch.  Each lane does f25_load,
 * the one call, f25_store of the raw (unreduced) result; only `freeze`
 * freezes.
 */
#include "launch.h"

#include "fe25519.h"

using namespace na;

namespace {

constexpr uint32_t F25_BLOCK = 64;

__global__ void __launch_bounds__(F25_BLOCK) f25_op_batch(int op, const uint8_t *a, const uint8_t *b, uint8_t *out,
                                                          uint32_t n)
{
    const uint32_t i = blockIdx.x * F25_BLOCK + threadIdx.x;
    if (i >= n) return;
    const F25 x = f25_load(a + (uint64_t)i * 32);
    F25 r;
    switch (op) {
    case NOISE_AEAD_F25_ADD: r = f25_add(x, f25_load(b + (uint64_t)i * 32)); break;
    case NOISE_AEAD_F25_SUB: r = f25_sub(x, f25_load(b + (uint64_t)i * 32)); break;
    case NOISE_AEAD_F25_MUL: r = f25_mul(x, f25_load(b + (uint64_t)i * 32)); break;
    case NOISE_AEAD_F25_SQ: r = f25_sq(x); break;
    case NOISE_AEAD_F25_MUL_121665: r = f25_mul_small(x, 121665u); break;
    case NOISE_AEAD_F25_MUL_9: r = f25_mul_small(x, 9u); break;
    case NOISE_AEAD_F25_FREEZE: r = f25_freeze(x); break;
    default: r = f25_invert(x); break;
    }
    f25_store(out + (uint64_t)i * 32, r);
}

bool meets(const uint8_t *p, const uint8_t *q, uint64_t bytes)
{
    const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
    return x < y ? y - x < bytes : x - y < bytes;
}

} // namespace

extern "C" int noise_aead_debug_f25_op(int op, const uint8_t *d_a, const uint8_t *d_b, uint32_t n, uint8_t *d_out,
                                       void *stream)
{
    if (op < NOISE_AEAD_F25_ADD || op > NOISE_AEAD_F25_INVERT) return NOISE_ERROR_UNKNOWN_ID;
    if (!n) return NOISE_ERROR_NONE;
    const bool binary = op <= NOISE_AEAD_F25_MUL;
    if (!d_a || !d_out || (binary && !d_b)) return NOISE_ERROR_INVALID_PARAM;
    const uint64_t bytes = (uint64_t)32 * n;
    if (meets(d_out, d_a, bytes) || (binary && meets(d_out, d_b, bytes))) return NOISE_ERROR_INVALID_PARAM;
    return launch_items(f25_op_batch, n, F25_BLOCK, (hipStream_t)stream, op, d_a, binary ? d_b : nullptr, d_out, n);
}
