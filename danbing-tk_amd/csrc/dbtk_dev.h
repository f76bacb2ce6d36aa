// dbtk_dev.h — the host plumbing of the side modules (dbtk_pred.hip, dbtk_kcp.hip, dbtk_sim.hip, dbtk_eval.hip, dbtk_assoc.hip): the
// one HIP status check, the owners of device arrays, streams and events, and the three questions every module asks of the runtime.
// A side module names a device pointer once, as an owner (a handle's member or a local): what the owner holds is freed on every way out
// of its scope, DEVCHK's returns included.  Host code only; dbtk_hip.hip has owners of its own (they go through its allocation trace).
#ifndef DBTK_DEV_H_
#define DBTK_DEV_H_

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <string>

#include "dbtk_internal.h"

#define DEVCHK(call)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            dbtk::set_error(std::string(#call) + ": " + hipGetErrorString(e_));                       \
            return DBTK_ERR_HIP;                                                                      \
        }                                                                                             \
    } while (0)

namespace dbtk {

// A device array and its capacity in elements.  alloc and reserve hand back the runtime's status: the module's wrapper of a few lines
// turns it into its own message and status, and decides how much more than `need` a grown buffer gets (`want`).
template <class T>
class DevArr {
public:
    DevArr() = default;
    DevArr(DevArr&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevArr& operator=(DevArr&& o) noexcept { if (this != &o) { drop(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
    ~DevArr() { drop(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }  // (a kernel argument, a copy's end: the owner reads as the pointer it holds)
    size_t cap() const { return cap_; }
    T* release() { T* r = p_; p_ = nullptr; cap_ = 0; return r; }
    void drop() { if (p_) (void)hipFree(p_); p_ = nullptr; cap_ = 0; }
    hipError_t alloc(size_t n) {  // what it held goes first: nothing is kept
        drop();
        const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
        if (e == hipSuccess) cap_ = n; else p_ = nullptr;
        return e;
    }
    hipError_t reserve(size_t need, size_t want) { return need <= cap_ ? hipSuccess : alloc(want); }
private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// A stream or an event; the flags are given where it is created.
template <class H, hipError_t (*CREATE)(H*, unsigned), hipError_t (*DESTROY)(H)>
class DevHandle {
public:
    DevHandle() = default;
    DevHandle(DevHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DevHandle& operator=(DevHandle&& o) noexcept { if (this != &o) { drop(); h_ = o.h_; o.h_ = nullptr; } return *this; }
    ~DevHandle() { drop(); }
    H get() const { return h_; }
    operator H() const { return h_; }
    hipError_t create(unsigned flags) {
        drop();
        const hipError_t e = CREATE(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
private:
    void drop() { if (h_) (void)DESTROY(h_); h_ = nullptr; }
    H h_ = nullptr;
};
using DevStream = DevHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;
using DevEvent = DevHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;

// the number of devices; none is an error (the range check and its message are the caller's)
inline dbtk_status_t device_count(int* ndev) {
    if (hipGetDeviceCount(ndev) == hipSuccess && *ndev > 0) return DBTK_OK;
    (void)hipGetLastError();
    set_error("no HIP device (the library has no CPU path)");
    return DBTK_ERR_NO_DEVICE;
}
// the compute units of a device, at least 1
inline hipError_t device_cus(int device, int* num_cu) {
    hipDeviceProp_t prop;
    const hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) *num_cu = prop.multiProcessorCount > 1 ? prop.multiProcessorCount : 1;
    return e;
}
inline bool is_device_memory_of(const void* p, int device) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == device) return true;
    (void)hipGetLastError();
    return false;
}

}  // namespace dbtk

#endif
