// Host-side helpers shared by the .hip files: error reporting, the current-device guard, device
// allocation and the compute-unit count. Host only; nothing here is device code.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "sa_hip.h"

namespace sa {

// Stores what sa_last_error() reports and returns `code`. The thread-local string is one object,
// in sa_engine.hip, for every translation unit.
int set_error(int code, const std::string &msg);

inline int fail(int code, const std::string &msg) { return set_error(code, msg); }

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return sa::fail(SA_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

// Makes `device` current for a scope and restores the caller's device on every return path.
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// Device buffer freed on every return path (one-shot calls, debug dumps).
template <typename T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};

// hipMalloc of at least 16 bytes, so that an empty buffer still has an address.
template <typename T>
int dmalloc(T **p, size_t bytes)
{
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    if (hipMalloc((void **)p, bytes) != hipSuccess)
    {
        (void)hipGetLastError();
        *p = nullptr;
        return fail(SA_ERR_NOMEM, "device allocation of " + std::to_string(bytes) + " bytes failed");
    }
    return SA_OK;
}

// Compute units of `device`, cached (hipGetDeviceProperties costs milliseconds per call).
inline int device_cus(int device)
{
    static std::mutex mu;
    static std::vector<int> cus;
    if (device < 0) return 256;  // no such device: the caller's DeviceGuard reports it
    std::lock_guard<std::mutex> lk(mu);
    if (device >= (int)cus.size()) cus.resize(device + 1, 0);
    if (cus[device] == 0)
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v <= 0)
        {
            (void)hipGetLastError();
            v = 256;
        }
        cus[device] = v;
    }
    return cus[device];
}

}  // namespace sa
