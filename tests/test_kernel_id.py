"""The kernel identity (csrc/kernel_id.hpp), without a GPU.

One value names a tracer kernel for the launchers, the occupancy cache, the
per-scene builds and the texts of errors and logs.  A wrong slot or index would
not fail: it would silently reuse another kernel's occupancy or another
variant's function.  A stand-alone program (plain g++: the header includes
nothing of HIP) prints every slot, index, name and text; the checks are here:

  - occupancy slots over every (family, pool, lds, precision) are distinct and
    below kOccupancySlots (the ray-batch family has no pool kernel);
  - per-scene variants over every (family but rays, pool, lds, no_skips, 7
    waves) are distinct and below kVariants;
  - is_optional holds exactly for the 7-wave, supersampled and lens variants;
  - name() gives the hipRTC name expressions written out below, four per
    family (the disk cache's key holds the name);
  - describe() gives the texts of the launch errors and the per-scene log.
"""
import itertools
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "ray-tracer-challenge-rs_amd", "csrc", "kernel_id.hpp")

PROGRAM = r"""
#include <cstdio>
#include "%s"
using namespace rtc;
int main() {
    static_assert(KernelId{}.occupancy_slot(false) >= 0, "constexpr");
    static_assert(KernelId{}.variant(false, false) >= 0, "constexpr");
    std::printf("limits %%d %%d\n", KernelId::kOccupancySlots, KernelId::kVariants);
    for (int f = 0; f < 4; ++f)
        for (int pool = 0; pool < 2; ++pool)
            for (int lds = 0; lds < 2; ++lds)
                for (int dup = 0; dup < 2; ++dup) {
                    KernelId id;
                    id.family = (KernelFamily)f, id.pool = pool, id.lds = lds, id.dup = dup;
                    const char* name = id.name();
                    std::printf("id %%d %%d %%d %%d|%%d %%d|%%s|%%s|", f, pool, lds, dup, id.occupancy_slot(false),
                                id.occupancy_slot(true), name ? name : "-", id.describe());
                    for (int ns = 0; ns < 2; ++ns)
                        for (int w7 = 0; w7 < 2; ++w7) {
                            const int v = id.variant(ns, w7);
                            std::printf(" %%d:%%d", v, v >= 0 && v < KernelId::kVariants ? (int)KernelId::is_optional(v) : -1);
                        }
                    std::printf("\n");
                }
    return 0;
}
"""

FRAME, SUPERSAMPLED, LENS, RAYS = range(4)

# what rtc_jit.cpp's kernel_name returned, by (family, pool, lds)
NAMES = {
    (FRAME, 0, 0): "rtc::trace_direct<float, false>",
    (FRAME, 0, 1): "rtc::trace_direct<float, true>",
    (FRAME, 1, 0): "rtc::trace_pool<float, false, false>",
    (FRAME, 1, 1): "rtc::trace_pool<float, true, false>",
    (SUPERSAMPLED, 0, 0): "rtc::trace_direct_ss<float, false>",
    (SUPERSAMPLED, 0, 1): "rtc::trace_direct_ss<float, true>",
    (SUPERSAMPLED, 1, 0): "rtc::trace_pool_ss<float, false, false>",
    (SUPERSAMPLED, 1, 1): "rtc::trace_pool_ss<float, true, false>",
    (LENS, 0, 0): "rtc::trace_direct_lens<float, false>",
    (LENS, 0, 1): "rtc::trace_direct_lens<float, true>",
    (LENS, 1, 0): "rtc::trace_pool_lens<float, false, false>",
    (LENS, 1, 1): "rtc::trace_pool_lens<float, true, false>",
}
# the prefixes of "launch of the ... kernel" and "per-scene ... kernel not used"
TEXTS = {
    (FRAME, 0): "direct", (FRAME, 1): "pool",
    (SUPERSAMPLED, 0): "supersampled direct", (SUPERSAMPLED, 1): "supersampled pool",
    (LENS, 0): "lens direct", (LENS, 1): "lens pool",
    (RAYS, 0): "ray-batch",
}


def table(tmp_path):
    src = tmp_path / "kernel_id.cpp"
    src.write_text(PROGRAM % os.path.abspath(HEADER))
    exe = tmp_path / "kernel_id"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    slots, variants = (int(v) for v in out[0].split()[1:])
    ids = {}
    for line in out[1:]:
        key, occ, name, text, var = line[3:].split("|")
        ids[tuple(int(v) for v in key.split())] = dict(
            occ=tuple(int(v) for v in occ.split()), name=name, text=text,
            variants=[tuple(int(v) for v in item.split(":")) for item in var.split()])
    assert len(ids) == 32
    return slots, variants, ids


def test_kernel_identity(tmp_path):
    n_slots, n_variants, ids = table(tmp_path)

    # occupancy slots: one per (family, pool, lds, precision), none for dup, dense enough for the arrays
    seen = {}
    for (f, pool, lds, dup), rec in ids.items():
        if f == RAYS and pool:
            continue  # not a kernel
        for f64, slot in enumerate(rec["occ"]):
            assert 0 <= slot < n_slots, (f, pool, lds, f64, slot)
            assert seen.setdefault(slot, (f, pool, lds, f64)) == (f, pool, lds, f64), "two kernels share slot %d" % slot
            assert slot == ids[(f, pool, lds, 0)]["occ"][f64]  # dup = true is planned with dup = false's occupancy
    assert len(seen) == 3 * 8 + 4 == n_slots  # every slot of the arrays is some kernel's

    # per-scene variants: (family but rays, pool, lds, no_skips, 7 waves), dup = false
    seen = {}
    for f, pool, lds in itertools.product((FRAME, SUPERSAMPLED, LENS), (0, 1), (0, 1)):
        for (no_skips, waves7), (v, optional) in zip(itertools.product((0, 1), (0, 1)), ids[(f, pool, lds, 0)]["variants"]):
            assert 0 <= v < n_variants, (f, pool, lds, no_skips, waves7, v)
            assert seen.setdefault(v, (f, pool, lds, no_skips, waves7)) == (f, pool, lds, no_skips, waves7)
            assert optional == int(bool(waves7) or f in (SUPERSAMPLED, LENS)), (f, pool, lds, no_skips, waves7)
    assert len(seen) == 3 * 2 * 2 * 2 * 2 == n_variants

    # names and texts, whatever dup says
    for (f, pool, lds, dup), rec in ids.items():
        assert rec["name"] == NAMES.get((f, pool, lds), "-"), (f, pool, lds, dup)
        if (f, pool) in TEXTS:
            assert rec["text"] == TEXTS[(f, pool)], (f, pool, lds, dup)
    assert len(set(NAMES.values())) == 12
