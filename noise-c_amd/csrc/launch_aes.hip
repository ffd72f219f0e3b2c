/*
 * launch_aes.hip — launcher of the AES-GCM kernels (aesgcm.hip): the
 * per-device table build, key preparation, and the launch of a Plan
 * (dispatch.h) as the instantiation it names.  Called by the C-ABI layer
 * (aead_api.hip) through launch.h.
 *
 * UniformArgs::vf and RaggedArgs::vf are ChaChaPoly's: the AES-GCM kernels
 * do not read them (but gcm_duplex_fused<true>, whose record body is kept as
 * it was, aesgcm.hip gcm_staged_rec_own; vf is always set there).  Every
 * AES-GCM open verifies first (dispatch.h open_vf) — it authenticates,
 * takes the verdict, then decrypts — because an AES-GCM open never writes a
 * byte of a rejected record (cipher-aesgcm.c:184-186), so the other kernels
 * compile no other order.
 */
#include "launch.h"
#include "transport_plan.h"
#include "aesgcm.hip"
#include <mutex>

namespace na {
namespace {

constexpr int kMaxDevices = 64;
std::mutex g_tab_mu[kMaxDevices];
bool g_tab_ready[kMaxDevices];

} // namespace

/* S-box / T-table are generated on each device once (aesgcm.hip), on a
   private stream — never the caller's, which may be capturing a graph —
   and waited for.  Only success is remembered: after a failure the next AES
   call on that device tries again. */
hipError_t ensure_aes_tables()
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    if (__atomic_load_n(&g_tab_ready[dev], __ATOMIC_ACQUIRE)) return hipSuccess;
    std::lock_guard<std::mutex> lk(g_tab_mu[dev]);
    if (g_tab_ready[dev]) return hipSuccess;
    hipStream_t s = nullptr;
    e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(aes_tables_init, dim3(1), dim3(256), 0, s);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    if (e == hipSuccess) __atomic_store_n(&g_tab_ready[dev], true, __ATOMIC_RELEASE);
    return e;
}

static_assert(PLAN_GCM_LANES == GCM_LANES && PLAN_GCM_WG == GCM_WG && PLAN_GCM_WG_RECS == GCM_WG_RECS,
              "dispatch.h counts grids with the kernels' geometry");

namespace {

using AnyKernel = void (*)();
template <typename... A>
AnyKernel any(void (*fn)(A...)) { return (AnyKernel)fn; }

template <bool CT, int WG, int R, int KL = GCM_LANES>
AnyKernel gcm_ragged_pick(bool open, bool fast)
{
    return any(open ? (fast ? gcm_ragged_staged<true, true, WG, CT, R, KL>
                            : gcm_ragged_staged<true, false, WG, CT, R, KL>)
                    : (fast ? gcm_ragged_staged<false, true, WG, CT, R, KL>
                            : gcm_ragged_staged<false, false, WG, CT, R, KL>));
}

/* the kernels whose template arguments are OPEN and CT */
#define NA_OPEN_CT(kernel) \
    any(p.ct ? (p.open ? kernel<true, true> : kernel<false, true>) : (p.open ? kernel<true, false> : kernel<false, false>))

/* The plan's kernel value and template arguments as the function pointer
   (nullptr: no such instantiation). */
template <bool CT>
AnyKernel gcm_ragged_kernel(const Plan &p)
{
    if (p.lanes == 8) return gcm_ragged_pick<CT, 1024, 2, 8>(p.open, p.fast);
    if (p.wg == 1024 && p.r == 2) return gcm_ragged_pick<CT, 1024, 2>(p.open, p.fast);
    if (p.wg == 1024) return gcm_ragged_pick<CT, 1024, 1>(p.open, p.fast);
    return gcm_ragged_pick<CT, 256, 1>(p.open, p.fast);
}

/* gcm_duplex_ragged in the shapes gcm_ragged_kernel picks */
template <bool CT, bool FAST>
AnyKernel gcm_duplex_ragged_kernel(const Plan &p)
{
    if (p.lanes == 8) return any(gcm_duplex_ragged<FAST, 1024, CT, 2, 8>);
    if (p.wg == 1024 && p.r == 2) return any(gcm_duplex_ragged<FAST, 1024, CT, 2>);
    if (p.wg == 1024) return any(gcm_duplex_ragged<FAST, 1024, CT, 1>);
    return any(gcm_duplex_ragged<FAST, 256, CT, 1>);
}

AnyKernel aes_kernel(const Plan &p)
{
    switch (p.kernel) {
    case K_GCM_UNIFORM: return NA_OPEN_CT(gcm_uniform);
    case K_GCM_STAGED: return NA_OPEN_CT(gcm_staged);
    case K_GCM_WIDE: return NA_OPEN_CT(gcm_wide);
    case K_GCM_DUPLEX_FUSED: return any(p.ct ? gcm_duplex_fused<true> : gcm_duplex_fused<false>);
    case K_GCM_DUPLEX_STAGED: return any(p.ct ? gcm_duplex_staged<true> : gcm_duplex_staged<false>);
    case K_GCM_RAGGED: return p.ct ? gcm_ragged_kernel<true>(p) : gcm_ragged_kernel<false>(p);
    case K_GCM_DUPLEX_RAGGED:
        if (p.ct) return p.fast ? gcm_duplex_ragged_kernel<true, true>(p) : gcm_duplex_ragged_kernel<true, false>(p);
        return p.fast ? gcm_duplex_ragged_kernel<false, true>(p) : gcm_duplex_ragged_kernel<false, false>(p);
    default: return nullptr;
    }
}
#undef NA_OPEN_CT

} // namespace

int aes_prepare(const uint8_t *raw_keys, uint32_t n_states, void *ctx, hipStream_t s)
{
    hipLaunchKernelGGL(gcm_prepare, dim3(n_states), dim3(256), 0, s, raw_keys, (AesCtx *)ctx, n_states);
    return hip_rc(hipGetLastError());
}

int aes_prepare_slots(const uint32_t *slots, uint32_t m, uint32_t n, const uint8_t *k1, const uint8_t *k2,
                      const uint8_t *status, bool initiator, void *ctx, hipStream_t s)
{
    if (!m) return NOISE_ERROR_NONE;
    if (m > 0x7fffffffu / 2) return NOISE_ERROR_INVALID_PARAM; /* 2m workgroups in one grid */
    const int rc = hip_rc(ensure_aes_tables());
    if (rc) return rc;
    hipLaunchKernelGGL(gcm_prepare_slots, dim3(2 * m), dim3(256), 0, s, slots, m, n, k1, k2, status,
                       initiator ? 1u : 0u, (AesCtx *)ctx);
    return hip_rc(hipGetLastError());
}

int aes_rekey_slots(const uint32_t *slots, uint32_t m, uint32_t n, uint32_t directions, const uint8_t *which,
                    const uint8_t *keyed, void *ctx, hipStream_t s)
{
    if (!m) return NOISE_ERROR_NONE;
    if (m > 0x7fffffffu / 2) return NOISE_ERROR_INVALID_PARAM; /* 2m workgroups in one grid */
    const int rc = hip_rc(ensure_aes_tables());
    if (rc) return rc;
    hipLaunchKernelGGL(gcm_rekey_slots, dim3(2 * m), dim3(256), 0, s, slots, m, n, directions, which, keyed, (AesCtx *)ctx);
    return hip_rc(hipGetLastError());
}

int aes_rekey_keys(const uint8_t *keys, uint32_t n, uint8_t *out, hipStream_t s)
{
    if (!n) return NOISE_ERROR_NONE;
    const int rc = hip_rc(ensure_aes_tables());
    return rc ? rc : launch_items(gcm_rekey_keys, n, GCM_REKEY_BLOCK, s, keys, out, n);
}

int aes_launch(const Plan &p, const PlanArgs &args, hipStream_t s)
{
    using UniformFn = void (*)(UniformArgs);
    using RaggedFn = void (*)(RaggedArgs);
    using DuplexFn = void (*)(UniformArgs, UniformArgs, uint32_t, uint32_t);
    using DuplexRaggedFn = void (*)(RaggedArgs, RaggedArgs, uint32_t, uint32_t);
    const AnyKernel fn = aes_kernel(p);
    switch (p.kernel) {
    case K_GCM_DUPLEX_FUSED:
    case K_GCM_DUPLEX_STAGED: return launch(p, (DuplexFn)fn, s, *args.a, *args.b, p.sb, p.ob);
    case K_GCM_WIDE:
    case K_GCM_RAGGED: return launch(p, (RaggedFn)fn, s, *args.r);
    case K_GCM_DUPLEX_RAGGED: return launch(p, (DuplexRaggedFn)fn, s, *args.r, *args.ro, p.sb, p.ob);
    default: return launch(p, (UniformFn)fn, s, *args.a);
    }
}

} // namespace na
