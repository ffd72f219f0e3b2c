/*
 * launch.h — the kernel launchers of each translation unit, as seen by the
 * C-ABI layer (aead_api.hip).  launch_chacha.hip holds the ChaChaPoly
 * kernels, launch_aes.hip the AES-GCM ones; they compile in parallel.  Each
 * launches the Plan that dispatch.h made of a job.  Also what every device
 * unit outside the AEAD kernels shares: the one-lane-per-item launch
 * (launch_items) and the allocation of a device object (DevArena).
 * Internal (hidden visibility); the public ABI is include/noise_aead_hip.h.
 */
#pragma once
#include "noise_aead_hip.h"
#include "aead_kernels.h"
#include "dispatch.h"
#include <hip/hip_runtime.h>

#define NA_HIDDEN __attribute__((visibility("hidden")))

namespace na {

inline int hip_rc(hipError_t e) { return e == hipSuccess ? NOISE_ERROR_NONE : NOISE_ERROR_SYSTEM; }

/* ---- worker.hip: before a batch launch of this many workgroups (asks the
   device's resident single-call workers to leave when it fills every CU) */
NA_HIDDEN void worker_park_for_batch(uint32_t workgroups);

/* The one launch: fn is the plan's kernel (nullptr: the plan names none this
   unit holds), args its arguments. */
template <typename... A>
int launch(const Plan &p, void (*fn)(A...), hipStream_t s, const A &...args)
{
    if (!fn) return NOISE_ERROR_INVALID_PARAM;
    if (!p.grid) return NOISE_ERROR_NONE;
    if (p.park) worker_park_for_batch(p.park);
    hipLaunchKernelGGL(fn, dim3(p.grid), dim3(p.block), 0, s, args...);
    return hip_rc(hipGetLastError());
}

/* The other launch: one lane per item, `items` of them in workgroups of
   `block` lanes; the grid is counted in 64 bits, so an item count near 2^32
   does not wrap.  Whether zero items launch at all is the caller's to say. */
template <typename... P, typename... A>
int launch_items(void (*fn)(P...), uint64_t items, uint32_t block, hipStream_t s, const A &...args)
{
    hipLaunchKernelGGL(fn, dim3((uint32_t)((items + block - 1) / block)), dim3(block), 0, s, args...);
    return hip_rc(hipGetLastError());
}

/* The one device allocation of a device object (handshake.hip,
   transport.hip).  carve() lays the parts out one after another, each padded
   to `align` (a power of two); alloc() makes the block, at() gives a part.
   What it holds is key material: zero() clears it on a stream before first
   use, and release() is the only way it goes. */
struct DevArena {
    uint8_t *mem;
    size_t bytes, align;

    size_t carve(size_t part)
    {
        const size_t at = bytes;
        bytes += (part + align - 1) & ~(align - 1);
        return at;
    }
    bool alloc() { return hipMalloc((void **)&mem, bytes) == hipSuccess; }
    template <typename T = uint8_t>
    T *at(size_t off) const { return (T *)(mem + off); }
    int zero(hipStream_t s) const { return hip_rc(hipMemsetAsync(mem, 0, bytes, s)); }
    /* Work of the object may still be in flight on the caller's streams, so
       wait, then zero, then free; the first error wins. */
    int release()
    {
        if (!mem) return NOISE_ERROR_NONE;
        const int rc = hip_rc(hipDeviceSynchronize());
        const int rc2 = hip_rc(hipMemset(mem, 0, bytes));
        const int rc3 = hip_rc(hipFree(mem));
        mem = nullptr;
        return rc ? rc : (rc2 ? rc2 : rc3);
    }
};

/* The arguments of a plan's kernel: a and b the (seal and open) jobs of a
   uniform or duplex plan, r the job of a ragged one, r and ro the seal and
   the open job of a ragged duplex; the others are null. */
struct PlanArgs {
    const UniformArgs *a, *b;
    const RaggedArgs *r, *ro;
};

/* ---- launch_chacha.hip */
NA_HIDDEN int chacha_launch(const Plan &p, const PlanArgs &args, hipStream_t s);
/* the current device's CU count (0: unknown), and its resident workgroups of
   a segmented ragged kernel — SEG_SEAL, SEG_OPEN: chachapoly_seg_ragged<open>,
   SEG_DUPLEX: chachapoly_seg_duplex: what the plans ask of the device */
enum SegKernel { SEG_SEAL, SEG_OPEN, SEG_DUPLEX };
NA_HIDDEN uint32_t device_cus();
NA_HIDDEN uint32_t seg_resident(SegKernel which);

/* ---- launch_aes.hip */
NA_HIDDEN int aes_launch(const Plan &p, const PlanArgs &args, hipStream_t s);
/* S-box / T-table of the current device, built once (private stream) */
NA_HIDDEN hipError_t ensure_aes_tables();
NA_HIDDEN int aes_prepare(const uint8_t *raw_keys, uint32_t n_states, void *ctx, hipStream_t s);
/* the contexts of a transport object's slots (transport.hip): entry j < m is
   slot slots[j] of n, keyed from k1 + 32 j and k2 + 32 j by role; ctx: n send
   contexts, then n receive ones.  Entries out of range or with a non-zero
   status byte (status may be null) are left alone.  Builds the tables first. */
NA_HIDDEN int aes_prepare_slots(const uint32_t *slots, uint32_t m, uint32_t n, const uint8_t *k1, const uint8_t *k2,
                                const uint8_t *status, bool initiator, void *ctx, hipStream_t s);
/* rekey of a transport object's slots (header section 12): entry j < m is slot
   slots[j] of n (slots may be null: slot j); the contexts of its directions
   directions & (which ? which[j] : 3) are rebuilt in place from REKEY of their
   own keys.  Entries out of range or with a zero byte in keyed (per slot) are
   left alone.  Builds the tables first. */
NA_HIDDEN int aes_rekey_slots(const uint32_t *slots, uint32_t m, uint32_t n, uint32_t directions, const uint8_t *which,
                              const uint8_t *keyed, void *ctx, hipStream_t s);
/* REKEY of n raw keys, 32 bytes apart, to out (which may be keys); builds the tables first */
NA_HIDDEN int aes_rekey_keys(const uint8_t *keys, uint32_t n, uint8_t *out, hipStream_t s);

} // namespace na
