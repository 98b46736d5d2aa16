// Host-side helpers shared by the .hip files: error reporting, the current-device guard, device
// allocation, the upload of host pairs and the compute-unit count. Host only; nothing here is device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
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

// The host pairs of a one-shot call packed back to back into two arenas, and the arenas on `device`:
// what every function that takes sa_host_pair does before it plans. `fn` is the C ABI function, for
// the message of a null sequence. The device is current only inside the call.
struct HostArenas {
    std::vector<sa_pair> pairs;  // the pairs as offsets into the arenas
    DevBuf<char> text, pattern;
};
inline int upload_host_pairs(const char *fn, const sa_host_pair *pairs, int64_t np, int device, HostArenas *out)
{
    out->pairs.resize((size_t)np);
    uint64_t tb = 0, pb = 0;
    for (int64_t p = 0; p < np; ++p)
    {
        if ((pairs[p].text_len && !pairs[p].text) || (pairs[p].pattern_len && !pairs[p].pattern))
            return fail(SA_ERR_INVALID, std::string(fn) + ": null sequence");
        out->pairs[p] = sa_pair{tb, pairs[p].text_len, pb, pairs[p].pattern_len};
        tb += pairs[p].text_len;
        pb += pairs[p].pattern_len;
    }
    DeviceGuard dg(device);
    if (!dg.ok) return fail(SA_ERR_HIP, "hipSetDevice failed");
    std::vector<char> ht(tb), hp(pb);
    for (int64_t p = 0; p < np; ++p)
    {
        if (pairs[p].text_len) std::memcpy(ht.data() + out->pairs[p].text_offset, pairs[p].text, pairs[p].text_len);
        if (pairs[p].pattern_len) std::memcpy(hp.data() + out->pairs[p].pattern_offset, pairs[p].pattern, pairs[p].pattern_len);
    }
    int rc;
    if ((rc = dmalloc(&out->text.p, tb)) || (rc = dmalloc(&out->pattern.p, pb))) return rc;
    if (tb) HIP_TRY(hipMemcpy(out->text.p, ht.data(), tb, hipMemcpyHostToDevice));
    if (pb) HIP_TRY(hipMemcpy(out->pattern.p, hp.data(), pb, hipMemcpyHostToDevice));
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
