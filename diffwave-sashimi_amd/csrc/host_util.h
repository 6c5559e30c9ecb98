// Host-side plumbing shared by the translation units: owners of the raw HIP resources (device and pinned memory,
// events, streams), the pinned staging ring of the per-call uploads, the content-keyed table upload, the stamp capture
// of the phase traces and the once-per-device setup of a kernel instance.  No device code.
#pragma once
#include <cstring>
#include <utility>
#include <vector>

#include "dws_common.h"

namespace dws {

// RAII device buffer.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    ~DevBuf() { release(); }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // (re)allocate when the request grows; contents are not preserved.
    int ensure(size_t n) {
        if (n <= bytes && p) return DWS_OK;
        release();
        if (n == 0) n = 4;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) {
            p = nullptr;
            return set_error(DWS_ERR_HIP, "hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
        }
        bytes = n;
        return DWS_OK;
    }
    float* f() const { return static_cast<float*>(p); }
};

// An event without timing, created on first use.
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    ~Event() {
        if (ev) (void)hipEventDestroy(ev);
    }
    int record(hipStream_t s) {
        if (!ev) DWS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        DWS_HIP(hipEventRecord(ev, s));
        return DWS_OK;
    }
    // what `s` enqueues from here on runs behind the last record (at once when there has been none)
    int make_wait(hipStream_t s) const {
        if (ev) DWS_HIP(hipStreamWaitEvent(s, ev, 0));
        return DWS_OK;
    }
    // the last record has completed (or there has been none); never waits
    bool done() const {
        if (!ev || hipEventQuery(ev) == hipSuccess) return true;
        (void)hipGetLastError();      // hipErrorNotReady is not an error
        return false;
    }
    int sync() const {
        if (ev) DWS_HIP(hipEventSynchronize(ev));
        return DWS_OK;
    }
};

// A non-blocking stream, created on first use.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    int get(hipStream_t* out) {
        if (!s) DWS_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        *out = s;
        return DWS_OK;
    }
};

// Pinned host memory.
struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    // grow to twice the request when it exceeds what is held; contents are not preserved.  A failed allocation leaves
    // the buffer as it was.
    int ensure(size_t n) {
        if (n <= bytes) return DWS_OK;
        void* q = nullptr;
        DWS_HIP(hipHostMalloc(&q, n * 2, hipHostMallocDefault));
        if (p) (void)hipHostFree(p);
        p = q;
        bytes = n * 2;
        return DWS_OK;
    }
};

// Pinned staging of a small per-call upload (a job table, labels, seeds), so that the copy never blocks the host:
//   void* h;  ring.acquire(bytes, &h);  <fill h>;  hipMemcpyAsync(dev, h, bytes, hipMemcpyHostToDevice, s);  ring.commit(s);
// acquire hands out the next slot whose last upload has been consumed (a query, no wait); while every slot is busy the
// ring grows, and only a full ring of `max_slots` busy slots makes the host wait, for the oldest.  commit records the
// slot's event behind the copy that reads it.
struct StagingRing {
    struct Slot {
        PinnedBuf buf;
        Event consumed;
    };
    std::vector<Slot> slots;
    int max_slots, next = 0, cur = -1;
    explicit StagingRing(int max_slots_) : max_slots(max_slots_) {}
    int acquire(size_t bytes, void** host) {
        const int n = (int)slots.size();
        int pick = -1;
        for (int k = 0; k < n && pick < 0; ++k)
            if (slots[(next + k) % n].consumed.done()) pick = (next + k) % n;
        if (pick < 0) {
            if (n < max_slots) {
                slots.emplace_back();
                pick = n;
            } else {
                pick = next % n;
                DWS_TRY(slots[pick].consumed.sync());
            }
        }
        next = pick + 1;
        DWS_TRY(slots[pick].buf.ensure(bytes));
        cur = pick;
        *host = slots[pick].buf.p;
        return DWS_OK;
    }
    int commit(hipStream_t s) { return slots[cur].consumed.record(s); }
};

// The device copy of a table is keyed on its CONTENTS (the same size with another schedule must not reuse it): uploaded
// only when `src` differs from `have`, the host copy of what is resident.
template <class T>
int upload_if_changed(DevBuf& dev, std::vector<T>& have, const T* src, size_t count, hipStream_t s) {
    if (dev.p && have.size() == count && std::memcmp(src, have.data(), count * sizeof(T)) == 0) return DWS_OK;
    DWS_TRY(dev.ensure(count * sizeof(T)));
    DWS_HIP(hipMemcpyAsync(dev.p, src, count * sizeof(T), hipMemcpyHostToDevice, s));
    DWS_HIP(hipStreamSynchronize(s));
    have.assign(src, src + count);
    return DWS_OK;
}

// Phase traces (tools only): `launch(stamps)` runs the stamped kernel instance on `s` with a zeroed device array of n
// 64-bit stamps; returns the stamps once the stream has drained.  Empty: the array could not be allocated, nothing ran.
template <class F>
std::vector<unsigned long long> capture_stamps(size_t n, hipStream_t s, F&& launch) {
    std::vector<unsigned long long> h;
    DevBuf d;
    if (hipMalloc(&d.p, n * 8) != hipSuccess) return h;
    (void)hipMemsetAsync(d.p, 0, n * 8, s);
    launch(static_cast<unsigned long long*>(d.p));
    (void)hipStreamSynchronize(s);
    h.resize(n);
    (void)hipMemcpy(h.data(), d.p, n * 8, hipMemcpyDeviceToHost);
    return h;
}

// Per-DEVICE launch state: hipFuncSetAttribute, the CU count and occupancy are properties of a device, not of the process --
// a "done once" flag / cached count is an array indexed by the current device's ordinal (one process per GPU is the product
// layout; a process that drives several GPUs still gets every device set up).
constexpr int DWS_MAX_DEVICES = 16;
inline int current_device_slot() {
    int d = 0;
    (void)hipGetDevice(&d);
    return ((unsigned)d < (unsigned)DWS_MAX_DEVICES) ? d : 0;
}

// Setup of kernel instance K on the current device, done by its first launch there and never again: the dynamic-LDS limit
// raised to `lds` bytes.  With `slots`: also the resident workgroups of the device, CU count x workgroups of `threads`
// threads per CU (a persistent grid), cached beside the flag; `who` names the launcher in the error text.
template <auto K>
int kernel_setup(size_t lds, int* slots = nullptr, int threads = 0, const char* who = "") {
    static int state[DWS_MAX_DEVICES] = {};      // 0: not set up; the slot count (1 when none was asked for)
    int& st = state[current_device_slot()];
    if (st == 0) {
        DWS_HIP(hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int n = 1;
        if (slots) {
            int dev = 0, ncu = 0, per_cu = 0;
            DWS_HIP(hipGetDevice(&dev));
            DWS_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
            DWS_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, K, threads, lds));
            DWS_CHECK(ncu > 0 && per_cu > 0, DWS_ERR_HIP, "%s: occupancy query returned %d x %d", who, ncu, per_cu);
            n = ncu * per_cu;
        }
        st = n;
    }
    if (slots) *slots = st;
    return DWS_OK;
}

// CU count of the current device (256 when the query fails), cached per device.
inline int cu_count() {
    static int count[DWS_MAX_DEVICES] = {};
    int& n = count[current_device_slot()];
    if (!n) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}

}  // namespace dws
