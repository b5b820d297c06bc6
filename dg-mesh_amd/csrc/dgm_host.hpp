// Host helpers of the extern "C" entry points outside c_api.hip (which formats its messages with its own variadic fail()).
#pragma once
#include "dgm_common.hpp"

namespace dgm {

// the entry point's return value after an error: `m` is what dgm_last_error() then returns
static inline int fail(const char* m) {
    set_last_error(m);
    return 1;
}
// ... and after its last launch: 0, or 1 with the launch error's text
static inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}
static inline unsigned blocks(long long n, int threads = 256) { return (unsigned)((n + threads - 1) / threads); }

}  // namespace dgm
