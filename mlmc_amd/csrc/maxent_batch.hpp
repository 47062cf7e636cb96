// Host-side helpers shared by the batched max-entropy solver (maxent_batch.hip) and the density entries (density.hip).
#pragma once
#include <string>

#include "common.hpp"

namespace mlmc {

// grow-only device workspace and pinned staging buffer of these entry points (calls are serialised by the API lock)
struct MebWorkspace {
    char *dev = nullptr;
    size_t dev_cap = 0;
    char *host = nullptr;
    size_t host_cap = 0;
    int reserve(size_t dev_bytes, size_t host_bytes) {
        hipStream_t st = rt().stream;
        if (dev_bytes > dev_cap) {
            MLMC_HIP_CHECK(wait_stream(st));
            if (dev) (void)hipFree(dev);
            dev = nullptr;
            dev_cap = 0;
            MLMC_HIP_CHECK(hipMalloc((void **)&dev, dev_bytes));
            dev_cap = dev_bytes;
        }
        if (host_bytes > host_cap) {
            MLMC_HIP_CHECK(wait_stream(st));
            if (host) (void)hipHostFree(host);
            host = nullptr;
            host_cap = 0;
            MLMC_HIP_CHECK(hipHostMalloc((void **)&host, host_bytes, hipHostMallocDefault));
            host_cap = host_bytes;
        }
        return 0;
    }
    // a large device workspace (Phi of a big batch: B Q R1 doubles) or pinned staging buffer (10^7 staged points) is not kept
    // beyond the call that needed it
    void trim(size_t keep_bytes) {
        if (host_cap > keep_bytes) {
            (void)wait_stream(rt().stream);
            (void)hipHostFree(host);
            host = nullptr;
            host_cap = 0;
        }
        if (dev_cap > keep_bytes) {
            (void)wait_stream(rt().stream);
            (void)hipFree(dev);
            dev = nullptr;
            dev_cap = 0;
        }
    }
};
constexpr size_t MEB_KEEP_BYTES = (size_t)256 << 20;
MebWorkspace &meb_ws();   // maxent_batch.hip: one workspace for all of them

inline size_t meb_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

inline int meb_fail(const char *fn, int i, const std::string &what) {
    return fail(std::string(fn) + ": problem " + std::to_string(i) + ": " + what);
}

}  // namespace mlmc
