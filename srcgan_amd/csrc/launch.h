// Host side of a kernel launch, shared by the launchers of the convolution and weight-gradient kernels: what every one of them
// needs around hipLaunchKernelGGL and none of them has a say in.  No device code.
#pragma once
#include "common.h"
#include <atomic>
#include <stdlib.h>

// "f32" / "bf16" / "f16": the element type inside a profiling class string
template <typename T>
static inline const char* sg_dtype_tag() { return sizeof(T) == 4 ? "f32" : (__is_same(T, __bf16) ? "bf16" : "f16"); }

// f(T{}) with T = the element type of dtype (checked by the caller: sg_dtype_ok), as in
//   return sg_dtype_dispatch(dtype, [&](auto t) { return launch<decltype(t)>(p, st); });
// The 16-bit form is for paths that have no fp32 instance (it instantiates none).
template <typename F>
static inline auto sg_dtype_dispatch16(int dtype, F&& f) { return dtype == SRCGAN_F16 ? f(_Float16{}) : f(__bf16{}); }
template <typename F>
static inline auto sg_dtype_dispatch(int dtype, F&& f) { return dtype == SRCGAN_F32 ? f(float{}) : sg_dtype_dispatch16(dtype, f); }

// SRCGAN_DBG: the cost-removal bits of a diagnostic build (ConvP::dbg); 0 in the production library, where sg_env answers nullptr
static inline int sg_dbg_flags() {
    static const char* e = sg_env("SRCGAN_DBG");
    return e ? atoi(e) : 0;
}

// Per-device launch state lives in fixed tables indexed by the HIP device index; a device beyond them is served uncached.
constexpr int SG_MAX_DEV = 64;

// HIP index of the calling thread's current device.  A launcher reads it once and hands it to the helpers below, so that no
// launch asks the runtime twice.
static inline int sg_current_device(int& dev) {
    SG_HIP(hipGetDevice(&dev));
    return 0;
}

// Compute units of device dev (0, with the error set, if the runtime refuses).  Two threads may both ask the runtime the first
// time; they store the same value.
static inline int sg_cu_count(int dev) {
    static std::atomic<int> ncu[SG_MAX_DEV];
    int n = 0;
    const bool cached = dev >= 0 && dev < SG_MAX_DEV;
    if (cached && (n = ncu[dev].load(std::memory_order_relaxed)) > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
        srcgan_set_error("hipDeviceGetAttribute(MultiprocessorCount) failed");
        return 0;
    }
    if (cached) ncu[dev].store(n, std::memory_order_relaxed);
    return n;
}

// Let kernel Kern take `bytes` of dynamic LDS on device dev, the current one.  The attribute belongs to (kernel, device), so the once-state
// is one bit per device in a mask that exists once per kernel VALUE: Kern is a template argument, not a function parameter -- all
// void(*)(ConvP) kernels share one pointer type, and a static keyed on the type would be shared between them.  Thread-safe without
// a lock: setting the attribute twice is harmless, so two threads that both find the bit clear both set it.
template <auto Kern>
static int sg_allow_lds(size_t bytes, int dev) {
    static std::atomic<unsigned long long> done{0};
    static_assert(SG_MAX_DEV <= 64, "one bit per device");
    const bool cached = dev >= 0 && dev < SG_MAX_DEV;
    const unsigned long long bit = cached ? 1ull << dev : 0;
    if (done.load(std::memory_order_acquire) & bit) return 0;
    SG_HIP(hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}
