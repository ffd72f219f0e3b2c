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

/* chachapoly_duplex_ragged<K, FAST, VF>: VF only where the standalone open
   has the two instantiations (FAST, K >= 4) */
template <int K, bool FAST>
AnyKernel duplex_ragged_k(const Plan &p)
{
    if constexpr (FAST && K >= 4) return any(p.vf_order ? chachapoly_duplex_ragged<K, true, true> : chachapoly_duplex_ragged<K, true, false>);
    else return any(chachapoly_duplex_ragged<K, FAST, false>);
}

template <bool FAST>
AnyKernel duplex_ragged_fn(const Plan &p)
{
    switch (p.lanes) {
    case 1: return duplex_ragged_k<1, FAST>(p);
    case 2: return duplex_ragged_k<2, FAST>(p);
    case 4: return duplex_ragged_k<4, FAST>(p);
    case 8: return duplex_ragged_k<8, FAST>(p);
    case 16: return duplex_ragged_k<16, FAST>(p);
    case 32: return duplex_ragged_k<32, FAST>(p);
    case 64: return duplex_ragged_k<64, FAST>(p);
    }
    return nullptr;
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
    case K_CHACHA_DUPLEX_RAGGED: return p.fast ? duplex_ragged_fn<true>(p) : duplex_ragged_fn<false>(p);
    case K_CHACHA_SEG_DUPLEX: return any(chachapoly_seg_duplex);
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

/* Resident workgroups of a segmented ragged kernel on the current device
   (CUs x occupancy), cached per device and kernel: the persistent grid and
   worker_park_for_batch take this count. */
uint32_t seg_resident(SegKernel which)
{
    constexpr int MAX_DEV = 64;
    static std::atomic<uint32_t> cache[MAX_DEV][3];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
    std::atomic<uint32_t> *c = dev < MAX_DEV ? &cache[dev][which] : nullptr;
    uint32_t v = c ? c->load(std::memory_order_relaxed) : 0;
    if (!v) {
        int per = 0;
        const hipError_t e =
            which == SEG_DUPLEX ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, chachapoly_seg_duplex, 256, 0)
            : which == SEG_OPEN ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, chachapoly_seg_ragged<true>, 256, 0)
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

/* A ragged duplex of two segmented jobs: both plans in one stream-ordered
   scratch block (header and map of the seal job, then of the open job),
   built by the same three plan kernels, then ONE persistent kernel over both
   (chachapoly_seg_duplex). */
int chacha_seg_duplex(const Plan &plan, const RaggedArgs &sa, const RaggedArgs &oa, hipStream_t s)
{
    const auto round256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t open_off = round256(SEG_MAP_OFF + (size_t)sa.n_records * SEG_KMAX * sizeof(uint32_t));
    const size_t bytes = open_off + SEG_MAP_OFF + (size_t)oa.n_records * SEG_KMAX * sizeof(uint32_t);
    uint8_t *scratch = nullptr;
    if (hipMallocAsync((void **)&scratch, bytes, s) != hipSuccess) return NOISE_ERROR_NO_MEMORY;
#ifdef NA_SEG_DEBUG
    {
        uint64_t r[2] = {(uint64_t)(uintptr_t)scratch, (uint64_t)(uintptr_t)scratch + bytes};
        (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_seg_arena), r, sizeof(r), 2 * sizeof(uint64_t),
                                     hipMemcpyHostToDevice, s);
    }
#endif
    SegPlanHdr *hdr[2] = {(SegPlanHdr *)scratch, (SegPlanHdr *)(scratch + open_off)};
    uint32_t *map[2] = {(uint32_t *)(scratch + SEG_MAP_OFF), (uint32_t *)(scratch + open_off + SEG_MAP_OFF)};
    const RaggedArgs *job[2] = {&sa, &oa};
    int rc = NOISE_ERROR_NONE;
    for (int i = 0; i < 2 && !rc; ++i) {
        const RaggedArgs &a = *job[i];
        rc = hip_rc(hipMemsetAsync(hdr[i], 0, sizeof(SegPlanHdr), s));
        if (rc) break;
        const uint32_t pb = (a.n_records + 1023) / 1024;
        hipLaunchKernelGGL(seg_plan_count, dim3(pb), dim3(1024), 0, s, a.recs, a.n_records, hdr[i]);
        hipLaunchKernelGGL(seg_plan_scan, dim3(1), dim3(64), 0, s, hdr[i]);
        hipLaunchKernelGGL(seg_plan_place, dim3(pb), dim3(1024), 0, s, a.recs, a.n_records, hdr[i], map[i], a.status);
        rc = hip_rc(hipGetLastError());
    }
    if (!rc)
        rc = launch(plan, chachapoly_seg_duplex, s, sa, oa, hdr[0], (const uint32_t *)map[0], hdr[1],
                    (const uint32_t *)map[1]);
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
    using DuplexRaggedFn = void (*)(RaggedArgs, RaggedArgs, uint32_t, uint32_t);
    const AnyKernel fn = chacha_kernel(p);
    switch (p.kernel) {
    case K_CHACHA_DUPLEX_SOLO: return launch(p, (DuplexRunFn)fn, s, *args.a, *args.b, p.sb, p.ob, p.run);
    case K_CHACHA_DUPLEX_STAGED: return launch(p, (DuplexFn)fn, s, *args.a, *args.b, p.sb, p.ob);
    case K_CHACHA_RAGGED: return launch(p, (RaggedFn)fn, s, *args.r);
    case K_CHACHA_SEG_RAGGED: return chacha_ragged_seg(p, *args.r, s);
    case K_CHACHA_DUPLEX_RAGGED: return launch(p, (DuplexRaggedFn)fn, s, *args.r, *args.ro, p.sb, p.ob);
    case K_CHACHA_SEG_DUPLEX: return chacha_seg_duplex(p, *args.r, *args.ro, s);
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
