/*
 * launch_chacha.hip — launcher of the ChaChaPoly kernels (chachapoly.hip,
 * chachapoly_seg.hip): turns a Plan (dispatch.h) into the instantiation it
 * names and launches it, and answers what the plans ask of the device.
 * Called by the C-ABI layer (aead_api.hip) through launch.h.
 */
#include "launch.h"
#include "chachapoly.hip"
#include "chachapoly_seg.hip"
#include <atomic>

namespace na {
namespace {

static_assert(PLAN_SEG_KMAX == SEG_KMAX, "dispatch.h counts the segmented grid with SEG_KMAX");

using AnyKernel = void (*)();
template <typename... A>
AnyKernel any(void (*fn)(A...)) { return (AnyKernel)fn; }

template <int K>
AnyKernel staged_k(const Plan &p)
{
    if (p.kernel == K_CHACHA_DUPLEX_STAGED)
        return any(p.ukey ? chachapoly_duplex_staged<K, true> : chachapoly_duplex_staged<K, false>);
    if (p.kernel == K_CHACHA_STAGED_VF)
        return any(p.ukey ? chachapoly_open_staged_vf<K, true> : chachapoly_open_staged_vf<K, false>);
    if (p.ukey) return any(p.open ? chachapoly_open_staged<K, true> : chachapoly_seal_staged<K, true>);
    return any(p.open ? chachapoly_open_staged<K, false> : chachapoly_seal_staged<K, false>);
}

template <int K, bool FAST>
AnyKernel generic_k(const Plan &p)
{
    if (p.kernel == K_CHACHA_UNIFORM) {
        /* no plan names these: a FAST job on 1, 4 or 8 lanes takes the one-lane
           or a staged kernel (their device code stays instantiated, as it was) */
        if (FAST && (K == 1 || K == 4 || K == 8)) return nullptr;
        return any(p.open ? chachapoly_open_uniform<K, FAST> : chachapoly_seal_uniform<K, FAST>);
    }
    if (!p.open) return any(chachapoly_seal_ragged<K, FAST>);
    if constexpr (K < 4) return any(chachapoly_open_ragged<K, FAST>);
    else if constexpr (FAST) return any(p.vf_order ? chachapoly_open_ragged<K, true, true> : chachapoly_open_ragged<K, true, false>);
    else return any(chachapoly_open_ragged<K, false, false>);
}

/* the generic-layout and wide-group kernels, uniform or ragged */
template <bool FAST>
AnyKernel generic_fn(const Plan &p)
{
    switch (p.lanes) {
    case 1: return generic_k<1, FAST>(p);
    case 2: return generic_k<2, FAST>(p);
    case 4: return generic_k<4, FAST>(p);
    case 8: return generic_k<8, FAST>(p);
    case 16: return generic_k<16, FAST>(p);
    case 32: return generic_k<32, FAST>(p);
    case 64: return generic_k<64, FAST>(p);
    }
    return nullptr;
}

/* The plan's kernel value and template arguments as the function pointer
   (nullptr: no such instantiation). */
AnyKernel chacha_kernel(const Plan &p)
{
    switch (p.kernel) {
    case K_CHACHA_UNIFORM:
    case K_CHACHA_RAGGED: return p.fast ? generic_fn<true>(p) : generic_fn<false>(p);
    case K_CHACHA_STAGED:
    case K_CHACHA_STAGED_VF:
    case K_CHACHA_DUPLEX_STAGED: return p.lanes == 4 ? staged_k<4>(p) : (p.lanes == 8 ? staged_k<8>(p) : nullptr);
    case K_CHACHA_SOLO:
        if (p.runs) {
            if (p.ukey) return any(p.open ? chachapoly_open_solo<true, true> : chachapoly_seal_solo<true, true>);
            return any(p.open ? chachapoly_open_solo<false, true> : chachapoly_seal_solo<false, true>);
        }
        if (p.ukey) return any(p.open ? chachapoly_open_solo<true, false> : chachapoly_seal_solo<true, false>);
        return any(p.open ? chachapoly_open_solo<false, false> : chachapoly_seal_solo<false, false>);
    case K_CHACHA_SEG2:
        if (p.open) return any(p.ukey ? chachapoly_seg2_uniform<true, true> : chachapoly_seg2_uniform<true, false>);
        return any(p.ukey ? chachapoly_seg2_uniform<false, true> : chachapoly_seg2_uniform<false, false>);
    case K_CHACHA_DUPLEX_SOLO: return any(p.ukey ? chachapoly_duplex_solo<true> : chachapoly_duplex_solo<false>);
    case K_CHACHA_SEG_RAGGED: return any(p.open ? chachapoly_seg_ragged<true> : chachapoly_seg_ragged<false>);
    default: return nullptr;
    }
}

} // namespace

/* the current device's CU count, cached per device (a host may mix GPU
   models); 0: unknown */
uint32_t device_cus()
{
    constexpr int MAX_DEV = 64;
    static std::atomic<uint32_t> cache[MAX_DEV];
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
    std::atomic<uint32_t> *c = dev < MAX_DEV ? &cache[dev] : nullptr; /* past the table: asked each time */
    uint32_t v = c ? c->load(std::memory_order_relaxed) : 0;
    if (!v && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) {
        v = (uint32_t)cus; /* idempotent: a racing thread stores the same value */
        if (c) c->store(v, std::memory_order_relaxed);
    }
    return v;
}

/* Resident workgroups of chachapoly_seg_ragged<open> on the current device
   (CUs x occupancy), cached per device: the persistent grid and
   worker_park_for_batch take this count. */
uint32_t seg_resident(bool open)
{
    constexpr int MAX_DEV = 64;
    static std::atomic<uint32_t> cache[MAX_DEV][2];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
    std::atomic<uint32_t> *c = dev < MAX_DEV ? &cache[dev][open ? 1 : 0] : nullptr;
    uint32_t v = c ? c->load(std::memory_order_relaxed) : 0;
    if (!v) {
        int per = 0;
        const hipError_t e = open ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, chachapoly_seg_ragged<true>, 256, 0)
                                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, chachapoly_seg_ragged<false>, 256, 0);
        if (e != hipSuccess || per < 1) return 0;
        v = device_cus() * (uint32_t)per; /* idempotent: a racing thread stores the same value */
        if (c) c->store(v, std::memory_order_relaxed);
    }
    return v;
}

namespace {

/* Ragged FAST batch through the segmented one-lane kernel: the plan (count,
   scan, place) in a stream-ordered scratch block, then the persistent
   kernel, then the scratch is freed (stream-ordered too). */
int chacha_ragged_seg(const Plan &plan, const RaggedArgs &a, hipStream_t s)
{
    const size_t bytes = SEG_MAP_OFF + (size_t)a.n_records * SEG_KMAX * sizeof(uint32_t);
    uint8_t *scratch = nullptr;
    if (hipMallocAsync((void **)&scratch, bytes, s) != hipSuccess) return NOISE_ERROR_NO_MEMORY;
    SegPlanHdr *p = (SegPlanHdr *)scratch;
#ifdef NA_SEG_DEBUG
    {
        uint64_t r[2] = {(uint64_t)(uintptr_t)scratch, (uint64_t)(uintptr_t)scratch + bytes};
        (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_seg_arena), r, sizeof(r), 2 * sizeof(uint64_t),
                                     hipMemcpyHostToDevice, s);
    }
#endif
    uint32_t *map = (uint32_t *)(scratch + SEG_MAP_OFF);
    int rc = hip_rc(hipMemsetAsync(p, 0, sizeof(SegPlanHdr), s));
    const uint32_t pb = (a.n_records + 1023) / 1024;
    if (!rc) {
        hipLaunchKernelGGL(seg_plan_count, dim3(pb), dim3(1024), 0, s, a.recs, a.n_records, p);
        hipLaunchKernelGGL(seg_plan_scan, dim3(1), dim3(64), 0, s, p);
        hipLaunchKernelGGL(seg_plan_place, dim3(pb), dim3(1024), 0, s, a.recs, a.n_records, p, map, a.status);
        rc = hip_rc(hipGetLastError());
    }
    if (!rc) {
        using SegFn = void (*)(RaggedArgs, SegPlanHdr *, const uint32_t *);
        rc = launch(plan, (SegFn)chacha_kernel(plan), s, a, p, (const uint32_t *)map);
    }
    (void)hipFreeAsync(scratch, s);
    return rc;
}

} // namespace

int chacha_launch(const Plan &p, const PlanArgs &args, hipStream_t s)
{
    using UniformFn = void (*)(UniformArgs);
    using RaggedFn = void (*)(RaggedArgs);
    using DuplexFn = void (*)(UniformArgs, UniformArgs, uint32_t, uint32_t);
    using DuplexRunFn = void (*)(UniformArgs, UniformArgs, uint32_t, uint32_t, uint32_t);
    const AnyKernel fn = chacha_kernel(p);
    switch (p.kernel) {
    case K_CHACHA_DUPLEX_SOLO: return launch(p, (DuplexRunFn)fn, s, *args.a, *args.b, p.sb, p.ob, p.run);
    case K_CHACHA_DUPLEX_STAGED: return launch(p, (DuplexFn)fn, s, *args.a, *args.b, p.sb, p.ob);
    case K_CHACHA_RAGGED: return launch(p, (RaggedFn)fn, s, *args.r);
    case K_CHACHA_SEG_RAGGED: return chacha_ragged_seg(p, *args.r, s);
    default: return launch(p, (UniformFn)fn, s, *args.a);
    }
}

} // namespace na

#ifdef NA_SEG_DEBUG
/* debug variant only: the caller's buffer range the segmented kernels may
   touch, and the accesses they skipped (address, kind << 56 | n << 40 | info) */
extern "C" int noise_aead_debug_seg_arena(uint64_t lo, uint64_t hi)
{
    uint64_t r[2] = {lo, hi};
    uint32_t z = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(na::g_seg_arena), r, sizeof(r), 0, hipMemcpyHostToDevice) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(na::g_seg_nviol), &z, sizeof(z), 0, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

extern "C" int noise_aead_debug_seg_viol(uint64_t *out, int n)
{
    uint32_t cnt = 0;
    if (hipMemcpyFromSymbol(&cnt, HIP_SYMBOL(na::g_seg_nviol), sizeof(cnt), 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (n > 64) n = 64;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(na::g_seg_viol), sizeof(uint64_t) * n, 0, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return (int)cnt;
}
#endif

#ifdef NA_SEG_TL
/* debug variant only: the per-wave cycle accounts of the last persistent
   ragged launch (chachapoly_seg.hip SegTL), summed over waves into out[8];
   reset != 0 zeroes them afterwards.  Returns the waves that ran. */
extern "C" int noise_aead_debug_seg_tl(uint64_t *out, int reset)
{
    static unsigned long long h[4096][8];
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(na::g_seg_tlw), sizeof(h), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    int waves = 0;
    for (int k = 0; k < 8; ++k) out[k] = 0;
    for (int w = 0; w < 4096; ++w) {
        if (!h[w][0]) continue;
        ++waves;
        for (int k = 0; k < 8; ++k) out[k] += h[w][k];
    }
    if (reset) {
        static unsigned long long z[4096][8];
        if (hipMemcpyToSymbol(HIP_SYMBOL(na::g_seg_tlw), z, sizeof(z), 0, hipMemcpyHostToDevice) != hipSuccess)
            return -1;
    }
    return waves;
}
#endif
