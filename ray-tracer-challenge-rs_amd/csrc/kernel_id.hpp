// kernel_id.hpp — the identity of a tracer kernel (host only, nothing of HIP).
//
// Which kernel a launch runs is four facts: the family (the frame kernels, the
// supersampled and the lens frame kernels, the ray-batch kernel), pool or
// direct, the world staged in LDS or read from global memory, and the
// containers walk for worlds with value-equal shapes (dup).  Every place that
// depends on the choice takes it from here: the instantiation a build of
// rtc_kernels.hip launches (kernel_of), the occupancy cache's slot
// (rt_context::occ_*), the per-scene builds' index (rt_context::Jit) and their
// hipRTC name, the tile order a launch keeps, and the texts of errors and logs.
// tests/test_kernel_id.py checks the indices and writes the texts out.
#pragma once

namespace rtc {

enum class KernelFamily : int {
    frame,         // trace_direct, trace_pool
    supersampled,  // trace_direct_ss, trace_pool_ss
    lens,          // trace_direct_lens, trace_pool_lens
    rays,          // trace_rays (no pool: one ray tree per lane)
    shutter,       // trace_direct_shutter, trace_pool_shutter (the motion build alone; no per-scene build)
};

struct KernelId {
    KernelFamily family = KernelFamily::frame;
    bool pool = false;  // the ray pool's kernel (worlds with secondary rays), else the direct one
    bool lds = false;   // the world tables staged in LDS
    bool dup = false;   // the containers walk by identity class (generic kernels only)

    // The supersampled and the lens kernels: a sample loop around the frame kernels' work.
    constexpr bool sampled() const {
        return family == KernelFamily::supersampled || family == KernelFamily::lens || family == KernelFamily::shutter;
    }

    // Slot of the occupancy cache: one per (family, pool, LDS world, precision).  dup has none of its own:
    // occupancy is asked of the dup = false instantiation (rtc_kernels.hip kernel_occupancy).  The ray-batch
    // family comes last and has no pool kernel, so the slots are dense.
    static constexpr int kOccupancySlots = 3 * 8 + 4;
    // (the shutter family's eight follow them: kOccupancyEntries sizes the cache)
    static constexpr int kOccupancyEntries = kOccupancySlots + 8;
    constexpr int occupancy_slot(bool f64) const {
        const int base = family == KernelFamily::shutter ? kOccupancySlots : (int)family * 8;
        return base + (pool ? 4 : 0) + (lds ? 2 : 0) + (f64 ? 1 : 0);
    }

    // Index of a per-scene build (f32, dup = false, no ray batches): the identity, RT_FLAG_NO_SKIPS and the
    // pool kernel's build for 7 waves/SIMD.
    static constexpr int kVariants = 3 * 16;
    constexpr int variant(bool no_skips, bool waves7) const {
        return (int)family * 16 + (waves7 ? 8 : 0) + (no_skips ? 4 : 0) + (pool ? 2 : 0) + (lds ? 1 : 0);
    }
    // A build whose failure refuses that variant alone: the 7-wave, the supersampled and the lens builds
    // (a failed frame build at the static occupancy keeps the generic kernel for the world).
    static constexpr bool is_optional(int variant) { return variant >= 16 || (variant & 8) != 0; }

    // The hipRTC name expression of the per-scene build (dup = false); null for a ray batch.
    constexpr const char* name() const {
        switch (family) {
            case KernelFamily::frame:
                if (pool) return lds ? "rtc::trace_pool<float, true, false>" : "rtc::trace_pool<float, false, false>";
                return lds ? "rtc::trace_direct<float, true>" : "rtc::trace_direct<float, false>";
            case KernelFamily::supersampled:  // builds of their own, named apart (the disk cache key holds the name)
                if (pool) return lds ? "rtc::trace_pool_ss<float, true, false>" : "rtc::trace_pool_ss<float, false, false>";
                return lds ? "rtc::trace_direct_ss<float, true>" : "rtc::trace_direct_ss<float, false>";
            case KernelFamily::lens:
                if (pool) return lds ? "rtc::trace_pool_lens<float, true, false>" : "rtc::trace_pool_lens<float, false, false>";
                return lds ? "rtc::trace_direct_lens<float, true>" : "rtc::trace_direct_lens<float, false>";
            case KernelFamily::rays: break;
            case KernelFamily::shutter: break;
        }
        return nullptr;
    }

    // For "launch of the <describe()> kernel" and "per-scene <describe()> kernel not used".
    constexpr const char* describe() const {
        switch (family) {
            case KernelFamily::frame: return pool ? "pool" : "direct";
            case KernelFamily::supersampled: return pool ? "supersampled pool" : "supersampled direct";
            case KernelFamily::lens: return pool ? "lens pool" : "lens direct";
            case KernelFamily::shutter: return pool ? "shutter pool" : "shutter direct";
            case KernelFamily::rays: break;
        }
        return "ray-batch";
    }
};

}  // namespace rtc
