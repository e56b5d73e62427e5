// Per-device launch state of libvgh.so, in one place: hipFuncSetAttribute and the occupancy query act on the CURRENT device, so whatever a launcher does
// "once" it does once per device id (a second engine on another GPU of the same process needs its own opt-in).  A launcher keeps one `static PerDevice`
// per kernel and goes through once_per_device: a failed attempt is not remembered (it is tried again at the next launch), and a device the table has no slot
// for -- an id of kMaxDevices or more, or a failed hipGetDevice -- is served every time and never borrows another device's slot.  Racing threads compute the
// same value.  The one exception is stem_pool.hip: its pooling kernels' LDS size varies with the map, so they opt in on every call that needs it.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <initializer_list>

namespace {

constexpr int kMaxDevices = 16;
constexpr int kNoSlot = -1;

// pure: what hipGetDevice answered -> the slot of the per-device tables, or kNoSlot
inline int device_slot(hipError_t query, int id) { return query == hipSuccess && id >= 0 && id < kMaxDevices ? id : kNoSlot; }
inline int current_slot() {
    int id = 0;
    const hipError_t query = hipGetDevice(&id);
    return device_slot(query, id);
}

struct PerDevice {  // a flag or a value per device; 0 = not there yet (static storage: zero-initialised)
    std::atomic<int> v[kMaxDevices];
};

// The slot's value, from `make()` if the slot has none yet.  make() returns 0 for "failed": nothing is stored and the next call runs it again.
// (No HIP call in here: tests/flame_plan_host.hip hands it a counting callable.)
template <typename F>
inline int once_per_device(PerDevice& state, int slot, F&& make) {
    if (slot != kNoSlot) {
        const int have = state.v[slot].load(std::memory_order_acquire);
        if (have) return have;
    }
    const int made = make();
    if (made && slot != kNoSlot) state.v[slot].store(made, std::memory_order_release);
    return made;
}

// more than 64 KiB of dynamic LDS takes an opt-in per kernel; the implicit-GEMM launchers opt in their two epilogue variants together
template <typename... K>
inline hipError_t opt_in_dynamic_lds(PerDevice& done, int bytes, K... kernels) {
    hipError_t err = hipSuccess;
    once_per_device(done, current_slot(), [&] {
        for (const void* k : {(const void*)kernels...}) {
            const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
            if (err == hipSuccess) err = e;
        }
        return err == hipSuccess ? 1 : 0;
    });
    return err;
}

// resident blocks per CU of a persistent tile-loop kernel (>= 1), with the opt-in its LDS needs
template <typename K>
inline int patch_blocks_per_cu(K kernel, int threads, int lds, PerDevice& cache) {
    return once_per_device(cache, current_slot(), [&] {
        int n = 0;
        if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)kernel, threads, lds) != hipSuccess || n < 1) n = 1;
        return n;
    });
}

}  // namespace
