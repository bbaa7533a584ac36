// ppenv_host.h — host-side plumbing shared by the translation units of libppenv: the error text, HIP call and launch checks,
// grid sizes, device selection and the handles' status word.  Internal and host-only: no part of the ABI (include/*.h), exports nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/ppenv.h"

void ppenv_set_error(const char* msg);   // ppenv.hip: the calling thread's ppenv_last_error() text

namespace {

__attribute__((format(printf, 1, 2))) inline void pp_set_errorf(const char* fmt, ...) {
    char msg[512];   // the size of the text ppenv_last_error() keeps
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    ppenv_set_error(msg);
}

// a HIP runtime call of an entry point: on failure the entry returns PPENV_EHIP with "<call> failed: <reason>"
#define PP_HIP(call)                                                         \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) {                                              \
            pp_set_errorf("%s failed: %s", #call, hipGetErrorString(e_));    \
            return PPENV_EHIP;                                               \
        }                                                                    \
    } while (0)

// after a kernel launch: PPENV_OK, or PPENV_EHIP with the site's own text
inline int pp_launched(const char* what) {
    if (hipGetLastError() == hipSuccess) return PPENV_OK;
    ppenv_set_error(what);
    return PPENV_EHIP;
}

// workgroups of `block` lanes that cover n items (n up to 2^31 - 1 table entries: the count is formed in 64 bits)
inline uint32_t pp_blocks_of(int64_t n, int block) { return (uint32_t)((n + block - 1) / block); }

// every entry point of a handle launches on the device the handle was created on, whatever the caller's current device is
inline int pp_use_device(int id) {
    int cur = -1;
    PP_HIP(hipGetDevice(&cur));
    if (cur != id) PP_HIP(hipSetDevice(id));
    return PPENV_OK;
}

// A handle's PPENV_STATUS_* bits: one word of pinned host memory mapped into the device.  Kernels write it through `dev`, the host
// reads it at its next call without a synchronisation.
struct PPStatusWord {
    uint32_t* host = nullptr;
    uint32_t* dev = nullptr;
    // on the current device, zeroed; false (and nothing allocated) when the runtime refuses
    bool alloc() {
        if (hipHostMalloc((void**)&host, sizeof(uint32_t), hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer((void**)&dev, host, 0) == hipSuccess) {
            *host = 0u;
            return true;
        }
        release();
        return false;
    }
    void release() {
        if (host) (void)hipHostFree(host);
        host = dev = nullptr;
    }
    uint32_t read() const { return host ? *(volatile uint32_t*)host : 0u; }
    // Entry points that read or advance the state refuse to go on once a kernel has reported a fault: PPENV_EDEVICE with the caller's
    // text, which may print the word (%x) and then what it means (%s).
    int refuse_if_set(const char* fmt) const {
        const uint32_t st = read();
        if (st == 0) return PPENV_OK;
        pp_set_errorf(fmt, st, (st & PPENV_STATUS_HANDOFF_TIMEOUT) ? "a step-kernel wave timed out waiting for its partner wave's LDS hand-off and did not store its envs" : "unknown fault");
        return PPENV_EDEVICE;
    }
};

}  // namespace
