// The one way to launch a kernel with dynamic LDS.  Such a kernel must be opted in per device (its maximum dynamic
// shared memory size, a function attribute) before its first launch; launch_lds<K, LDS>() puts (K, LDS) into a
// process-wide table when the library is loaded (no HIP call), and swiftly_hip_create sets the attribute of every entry
// once per device.  The instances that exist and the LDS each needs are therefore written down once: at the launch.
// One LDS size per kernel instance: an instance launched with two sizes would be registered twice, and the attribute set
// last -- possibly the smaller -- would hold.
// Launches without dynamic LDS (a literal 0) stay plain hipLaunchKernelGGL calls.
#pragma once
#include <hip/hip_runtime.h>

namespace swf {

// the table (swiftly_abi_util.hip: one translation unit, behind a function-local static, so that the registrations of all
// kernel translation units land in it whatever their static-initialisation order)
bool register_kernel_lds(const void* host_fn, int lds_bytes);
// sets the attribute of every entry on the current device; returns the first error and the LDS size of its entry
int set_registered_kernel_attributes(int* failed_lds_bytes);

template <auto K, int LDS>
struct KernelLds {
    static inline const bool registered = register_kernel_lds((const void*)K, LDS);
};

// returns the launch status (a hipError_t)
template <auto K, size_t LDS, class... A>
inline int launch_lds(dim3 grid, dim3 block, hipStream_t s, const A&... args) {
    static_assert(LDS <= 160 * 1024, "LDS per workgroup");  // MI355X: 160 KiB per CU
    if constexpr (LDS > 0) (void)KernelLds<K, (int)LDS>::registered;
    hipLaunchKernelGGL(K, grid, block, LDS, s, args...);
    return (int)hipGetLastError();
}

}  // namespace swf
