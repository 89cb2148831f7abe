// What the multi-tensor launches (optim.hip: the optimizer step; grad_bucket.hip: the gradient bucket's pack) share: the chunk list
// over a set of tensors and the pinned staging ring their tables travel through.
//
// Chunk list.  A tensor is cut into chunks of kOptimChunk elements (tuning.h); prefix[t] is the number of chunks in front of tensor t,
// prefix[n] the total.  A workgroup takes chunk c, c + gridDim.x, ... and finds c's tensor with a binary search over prefix --
// wave-uniform, so scalar loads -- and nothing is looked up per element.
//
// Staging.  The table (records + prefix sums) is filled in a pinned slot of the library and copied to the caller's workspace on the
// call's stream, so the caller's descriptor array is dead when the call returns and the call does not wait for the stream (a copy from
// pageable memory would).  A ring of slots per device, each guarded by an event recorded behind its copy, keeps a call from
// overwriting a table whose copy is still queued; a slot is waited for only when kRing calls are in flight at once.  One ring serves
// both units (the variables are inline: one instance in the library).
#pragma once
#include <mutex>

#include "common.h"
#include "tuning.h"

namespace aspire {

inline int64_t chunks_of(int64_t n) { return (n + kOptimChunk - 1) / kOptimChunk; }

#ifdef __HIPCC__
// the tensor of chunk c: the last t with prefix[t] <= c (a tensor of no elements has no chunk and is never found); prefix[0] == 0 <= c,
// so the result is >= 0
__device__ __forceinline__ int chunk_tensor(const int32_t* __restrict__ prefix, int n_tensors, int c) {
    int lo = 0, hi = n_tensors;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] > c) hi = mid; else lo = mid + 1;
    }
    return lo - 1;
}
#endif

constexpr int kRing = 8, kMaxDevices = 64;
struct StagingSlot {
    void* host = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
};
struct StagingRing {
    StagingSlot slot[kRing];
    unsigned next = 0;
};
inline StagingRing g_staging_rings[kMaxDevices];
inline std::mutex g_staging_mu;

// One table's way to the device: acquire() hands out the current device's next slot, grown to `need` bytes and no longer in use;
// the caller fills host(); commit() queues the copy to `ws` on `st` and records the slot's event.  The ring's lock is held from
// acquire() to the end of the object's life, launch included, as the optimizer step always held it.
class Staging {
public:
    int acquire(const char* who, size_t need) {
        int dev = 0;
        ASPIRE_HIP_OK(hipGetDevice(&dev));
        ASPIRE_REQUIRE(dev >= 0 && dev < kMaxDevices, ASPIRE_ERR_UNSUPPORTED, "%s: device %d beyond the %d staging rings", who, dev,
                       kMaxDevices);
        lock_ = std::unique_lock<std::mutex>(g_staging_mu);
        StagingRing& ring = g_staging_rings[dev];
        StagingSlot& s = ring.slot[ring.next];
        ring.next = (ring.next + 1) % kRing;
        if (s.pending) {
            ASPIRE_HIP_OK(hipEventSynchronize(s.done));
            s.pending = false;
        }
        if (s.cap < need) {
            if (s.host) ASPIRE_HIP_OK(hipHostFree(s.host));
            s.host = nullptr;
            s.cap = 0;
            size_t cap = 16384;
            while (cap < need) cap *= 2;
            ASPIRE_HIP_OK(hipHostMalloc(&s.host, cap, hipHostMallocDefault));
            s.cap = cap;
        }
        if (!s.done) ASPIRE_HIP_OK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        slot_ = &s;
        need_ = need;
        return ASPIRE_OK;
    }
    void* host() const { return slot_->host; }
    int commit(void* ws, hipStream_t st) {
        ASPIRE_HIP_OK(hipMemcpyAsync(ws, slot_->host, need_, hipMemcpyHostToDevice, st));
        ASPIRE_HIP_OK(hipEventRecord(slot_->done, st));
        slot_->pending = true;
        return ASPIRE_OK;
    }

private:
    std::unique_lock<std::mutex> lock_;
    StagingSlot* slot_ = nullptr;
    size_t need_ = 0;
};

}  // namespace aspire
