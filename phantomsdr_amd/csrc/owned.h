// owned.h - internal: move-only owners of the four kinds of HIP resource the library creates (device buffer, pinned host
// buffer, event, stream).  An owner converts implicitly to the raw handle, so kernel argument structs, launches, pointer
// arithmetic and `if (c->d_wfout)` read as they would with a raw member; it releases what it holds when it dies (the HIP
// status is ignored, as in any destructor).  Creation reports through psdr_fail() and never throws; it REPLACES what the
// owner held only once the new resource exists, so a failed call leaves the owner as it was.  A member that only points
// at something owned elsewhere stays a raw pointer.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/psdr.h"

int psdr_fail(int code, const char *fmt, ...);

namespace psdr {

template <typename H, hipError_t (*Release)(H)>
class Owned {
   public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            reset(o.h_);
            o.h_ = nullptr;
        }
        return *this;
    }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }
    void reset(H fresh = nullptr) {  // (takes ownership of `fresh`)
        if (h_) Release(h_);
        h_ = fresh;
    }
    operator H() const { return h_; }
    H get() const { return h_; }  // where a cast to another pointer type follows

   protected:
    // the end of every create / alloc: keep `fresh` if `e` says it exists
    int adopt(hipError_t e, H fresh, const char *what) {
        if (e != hipSuccess) return psdr_fail(PSDR_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
        reset(fresh);
        return PSDR_OK;
    }

   private:
    H h_ = nullptr;
};

template <typename T>
hipError_t dev_release(T *p) { return hipFree(p); }
template <typename T>
hipError_t host_release(T *p) { return hipHostFree(p); }
// never fewer than 16 bytes: a buffer sized by a count that may be 0 still exists
template <typename T>
size_t buf_bytes(size_t count) { return std::max<size_t>(count * sizeof(T), 16); }

// `count` elements of T in device memory, cleared if `zero`
template <typename T>
struct DevBuf : Owned<T *, dev_release<T>> {
    int alloc(size_t count, bool zero = false) {
        T *p = nullptr;
        hipError_t e = hipMalloc((void **)&p, buf_bytes<T>(count));
        if (e == hipSuccess && zero && (e = hipMemset(p, 0, buf_bytes<T>(count))) != hipSuccess) hipFree(p);
        return this->adopt(e, p, "device allocation");
    }
};
// ... in pinned host memory
template <typename T>
struct HostBuf : Owned<T *, host_release<T>> {
    int alloc(size_t count) {
        T *p = nullptr;
        return this->adopt(hipHostMalloc((void **)&p, buf_bytes<T>(count), hipHostMallocDefault), p, "pinned host allocation");
    }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    // (an event belongs to the device that is current when it is created)
    int create(unsigned flags = hipEventDisableTiming) {
        hipEvent_t e = nullptr;
        return adopt(hipEventCreateWithFlags(&e, flags), e, "event creation");
    }
    int create_timing() { return create(hipEventDefault); }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    int create() {  // non-blocking, default priority
        hipStream_t s = nullptr;
        return adopt(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), s, "stream creation");
    }
    int create(int priority) {
        hipStream_t s = nullptr;
        return adopt(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority), s, "stream creation");
    }
};

}  // namespace psdr
