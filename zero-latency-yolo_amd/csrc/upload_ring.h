// upload_ring.h -- how a call's small host-built table (a grouping, a tile table, frame records) reaches the kernel that reads it without any call
// waiting for the device.  Host only; nothing but the HIP runtime API.
//
// A ring has DEPTH entries with one event each.  A call claims the next entry, fills it, uploads it in stream order, launches the work that reads
// it and marks the entry: its event is recorded behind that work.  An entry is rewritten only after the work that read it has completed -- claim
// synchronises with the entry's event, which by then lies DEPTH calls back and has long completed.  `last` is the entry marked most recently: the work
// of a ring's calls may run on different streams, and wait_last orders a stream behind the most recent of it.
//
//   SlotRing     the discipline alone: events, marks, cursor (the descriptor uploads of set_desc, whose device copy is single; zly_change_reset);
//                claim_behind_last is the claim of calls that are chained among themselves (the change map's, camera motion's)
//   UploadRing   ... plus the storage: DEPTH pinned host records mirrored by DEPTH device records of the same size
//
// Every operation returns the HIP error of the call that failed (hipSuccess otherwise); none is thread-safe: the owner's lock covers them.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace zly {

struct SlotRing {
    static constexpr int DEPTH = 8;
    hipEvent_t ev[DEPTH] = {};        // behind the work that read entry r
    bool used[DEPTH] = {};
    int next = 0, last = -1;          // last: the entry marked most recently, -1 = none yet

    hipError_t create()
    {
        hipError_t r = hipSuccess;
        for (int i = 0; i < DEPTH && r == hipSuccess; ++i) r = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        return r;
    }
    // also after a create that failed half way; returns the first error met
    hipError_t destroy()
    {
        hipError_t first = hipSuccess;
        for (int i = 0; i < DEPTH; ++i) {
            const hipError_t r = ev[i] ? hipEventDestroy(ev[i]) : hipSuccess;
            if (first == hipSuccess) first = r;
            ev[i] = nullptr; used[i] = false;
        }
        next = 0; last = -1;
        return first;
    }
    // *r = the next entry, free to be rewritten once this returns hipSuccess
    hipError_t claim(int* r)
    {
        *r = next;
        next = (next + 1) % DEPTH;
        return used[*r] ? hipEventSynchronize(ev[*r]) : hipSuccess;
    }
    // claim for work on s that must also run behind the entry marked most recently (calls that share scratch or state whichever streams they run
    // on): the entry is synchronised and s made to wait first, and the cursor advances only then -- a call that fails here leaves the ring as it was
    hipError_t claim_behind_last(hipStream_t s, int* r)
    {
        *r = next;
        if (used[*r])
            if (const hipError_t e = hipEventSynchronize(ev[*r])) return e;
        if (const hipError_t e = wait_last(s)) return e;
        next = (next + 1) % DEPTH;
        return hipSuccess;
    }
    // entry r's event behind what has been enqueued on s
    hipError_t mark(int r, hipStream_t s)
    {
        const hipError_t e = hipEventRecord(ev[r], s);
        if (e != hipSuccess) return e;
        used[r] = true;
        last = r;
        return hipSuccess;
    }
    // s behind the entry marked most recently
    hipError_t wait_last(hipStream_t s) const { return last >= 0 ? hipStreamWaitEvent(s, ev[last], 0) : hipSuccess; }
    // the work behind every mark made so far has completed
    hipError_t drain() const
    {
        for (int r = 0; r < DEPTH; ++r)
            if (used[r])
                if (const hipError_t e = hipEventSynchronize(ev[r])) return e;
        return hipSuccess;
    }
};

struct UploadRing : SlotRing {
    unsigned char* h = nullptr;       // pinned [DEPTH][entry_bytes]
    unsigned char* d = nullptr;       // device [DEPTH][entry_bytes]
    size_t entry_bytes = 0;

    hipError_t create(size_t bytes_per_entry)
    {
        entry_bytes = bytes_per_entry;
        if (const hipError_t e = hipMalloc((void**)&d, entry_bytes * DEPTH)) return e;
        if (const hipError_t e = hipHostMalloc((void**)&h, entry_bytes * DEPTH, hipHostMallocDefault)) return e;
        return SlotRing::create();
    }
    hipError_t destroy()
    {
        hipError_t first = d ? hipFree(d) : hipSuccess;
        const hipError_t rh = h ? hipHostFree(h) : hipSuccess, re = SlotRing::destroy();
        if (first == hipSuccess) first = rh;
        if (first == hipSuccess) first = re;
        d = nullptr; h = nullptr;
        return first;
    }
    // entry r as the caller's records, on the host and on the device
    template <typename T> T* host(int r) const { return reinterpret_cast<T*>(h + (size_t)r * entry_bytes); }
    template <typename T> T* dev(int r) const { return reinterpret_cast<T*>(d + (size_t)r * entry_bytes); }
    // the first `bytes` of entry r to the device, in s's order
    hipError_t upload(int r, size_t bytes, hipStream_t s) { return hipMemcpyAsync(dev<void>(r), host<void>(r), bytes, hipMemcpyHostToDevice, s); }
};

}  // namespace zly
