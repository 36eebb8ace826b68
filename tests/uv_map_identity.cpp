// CPU checks of the host side of texture maps (csrc/instances.hpp
// validate_maps and canonical_image_patterns with a map list, and
// csrc/shape_identity.hpp pattern_eq on the result), compiled stand-alone by
// tests/test_uv_maps_cpu.py, with the address and undefined-behaviour
// sanitizers where the compiler has them.  Prints one line per check and "ok".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../ray-tracer-challenge-rs_amd/csrc/instances.hpp"
#include "../ray-tracer-challenge-rs_amd/csrc/rtc_internal.hpp"

using namespace rtc;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            ++g_failed;                                   \
        }                                                 \
    } while (0)

static rt_pattern_desc pattern(int32_t kind, int32_t texture, int32_t filter) {
    rt_pattern_desc p;
    std::memset(&p, 0, sizeof p);
    p.kind = kind;
    p.sub_a = texture;
    p.sub_b = -1;
    p.reserved = filter;
    for (int i = 0; i < 16; ++i) p.inverse[i] = i % 5 == 0 ? 1.0 : 0.0;
    return p;
}
static rt_uv_map_desc map_of(uint32_t pattern, uint32_t map, std::vector<int32_t> faces = {-1, -1, -1, -1, -1, -1}) {
    rt_uv_map_desc m;
    m.pattern = pattern;
    m.map = map;
    for (int f = 0; f < 6; ++f) m.faces[f] = faces[f];
    return m;
}

int main() {
    // ---- 1: the refusals, each with its own text
    {
        const std::vector<rt_pattern_desc> pats = {pattern(RT_PATTERN_IMAGE, 0, 0), pattern(RT_PATTERN_STRIPE, -1, 0),
                                                   pattern(RT_PATTERN_IMAGE, 1, 1)};
        auto why = [&](std::vector<rt_uv_map_desc> list) {
            return inst::validate_maps(list.data(), (uint32_t)list.size(), pats.data(), (uint32_t)pats.size(), 3);
        };
        CHECK(why({}).empty(), "an empty list passes");
        CHECK(why({map_of(0, RT_MAP_SPHERICAL), map_of(2, RT_MAP_CUBE, {0, 1, 2, 2, 1, 0})}).empty(), "a well-formed list passes");
        CHECK(why({map_of(0, RT_MAP_PLANAR), map_of(2, RT_MAP_CYLINDRICAL)}).empty(), "planar and cylindrical pass");
        CHECK(inst::validate_maps(nullptr, 2, pats.data(), 3, 3) == "rt_scene_upload_mapped: null map list with nonzero count", "null list");
        CHECK(why({map_of(3, RT_MAP_SPHERICAL)}) == "map 0: pattern index out of range", "pattern index");
        CHECK(why({map_of(0, 1), map_of(1, RT_MAP_SPHERICAL)}) == "map 1: the pattern is not an image pattern", "not kind 6");
        CHECK(why({map_of(2, 1), map_of(0, 2), map_of(2, 1)}) == "map 2: pattern named twice", "twice");
        CHECK(why({map_of(0, 4)}) == "map 0: unknown map", "unknown map");
        CHECK(why({map_of(0, 0xFFFFFFFFu)}) == "map 0: unknown map", "unknown map, all bits");
        CHECK(why({map_of(0, RT_MAP_CUBE, {0, 1, 2, 3, 1, 0})}) == "map 0: face texture index out of range", "face 3 of 3 textures");
        CHECK(why({map_of(0, RT_MAP_CUBE, {0, 1, 2, -1, 1, 0})}) == "map 0: face texture index out of range", "face -1 of a cube map");
        CHECK(why({map_of(0, RT_MAP_SPHERICAL, {-1, -1, 0, -1, -1, -1})}) == "map 0: a face other than -1 for a map that is no cube map",
              "a face of a spherical map");
        CHECK(why({map_of(0, RT_MAP_PLANAR, {-1, -1, -1, -1, -1, 2})}) == "map 0: a face other than -1 for a map that is no cube map",
              "a face of a planar map");
        CHECK(inst::validate_maps(nullptr, 0, nullptr, 0, 0).empty(), "nothing at all passes");
        std::printf("refusals: 14 cases\n");
    }

    // ---- 2: the map takes part in a pattern's value; a planar entry is no entry
    const uint8_t pa[6] = {1, 2, 3, 4, 5, 6}, pb[6] = {1, 2, 3, 4, 5, 6}, pc[6] = {9, 2, 3, 4, 5, 200}, pd[3] = {7, 8, 90};
    // textures 0 and 1 hold one picture, 2 another, 3 a third (1 x 1)
    const rt_texture_desc tex[4] = {{pa, 2, 1}, {pb, 2, 1}, {pc, 2, 1}, {pd, 1, 1}};
    {
        std::vector<rt_pattern_desc> pats(5, pattern(RT_PATTERN_IMAGE, 0, 0));
        pats[1].sub_a = 1;
        const std::vector<rt_uv_map_desc> maps = {map_of(0, RT_MAP_SPHERICAL), map_of(1, RT_MAP_SPHERICAL), map_of(2, RT_MAP_CYLINDRICAL),
                                                  map_of(3, RT_MAP_PLANAR)};
        std::vector<int32_t> records = {5};
        inst::canonical_image_patterns(pats.data(), 5, tex, 4, maps.data(), 4, &records);
        CHECK(records.empty(), "no cube map: no record");
        CHECK(ident::pattern_eq(pats.data(), 0, 1), "two spherical maps over equal pictures");
        CHECK(!ident::pattern_eq(pats.data(), 0, 2), "spherical against cylindrical");
        CHECK(!ident::pattern_eq(pats.data(), 0, 3) && !ident::pattern_eq(pats.data(), 2, 4), "a map against the planar map");
        CHECK(ident::pattern_eq(pats.data(), 3, 4), "the planar map named and not named");
        CHECK((pats[0].reserved & 0xFF) == 0 && (pats[0].reserved >> 8) == RT_MAP_SPHERICAL && pats[4].reserved == 0, "the map beside the filter");
        std::printf("maps: part of a pattern's value\n");
    }

    // ---- 3: cube maps compare by their faces' pictures, whichever indices name them
    {
        std::vector<rt_pattern_desc> pats(5, pattern(RT_PATTERN_IMAGE, 0, 1));
        pats[1].sub_a = 1;
        pats[4].kind = RT_PATTERN_STRIPE;
        const std::vector<rt_uv_map_desc> maps = {
            map_of(1, RT_MAP_CUBE, {1, 0, 2, 3, 1, 0}),  // (named out of order: the list is sparse)
            map_of(0, RT_MAP_CUBE, {0, 1, 2, 3, 0, 1}),  // other indices, equal pictures
            map_of(2, RT_MAP_CUBE, {0, 0, 2, 3, 0, 2}),  // the last face differs
            map_of(3, RT_MAP_CUBE, {3, 3, 3, 3, 3, 3})};
        std::vector<int32_t> records;
        inst::canonical_image_patterns(pats.data(), 5, tex, 4, maps.data(), 4, &records);
        CHECK(records.size() == 3 * inst::kCubeRecords, "three distinct cube maps, got %zu records", records.size());
        const int32_t want[21] = {0, 0, 0, 2, 3, 0, 0, /**/ 0, 0, 0, 2, 3, 0, 2, /**/ 0, 3, 3, 3, 3, 3, 3};
        for (size_t i = 0; i < records.size() && i < 21; ++i) CHECK(records[i] == want[i], "record %zu: %d", i, records[i]);
        CHECK(pats[0].sub_a == 4 && pats[1].sub_a == 4 && pats[2].sub_a == 4 + 7 && pats[3].sub_a == 4 + 14, "records named: %d %d %d %d",
              pats[0].sub_a, pats[1].sub_a, pats[2].sub_a, pats[3].sub_a);
        CHECK(ident::pattern_eq(pats.data(), 0, 1), "faces with different indices and equal pictures");
        CHECK(!ident::pattern_eq(pats.data(), 0, 2), "one face differs");
        CHECK(!ident::pattern_eq(pats.data(), 0, 3), "every face differs");
        // the brightness bound: the largest channel over the six faces (and the pattern's own texture)
        CHECK(pats[0].color_a[0] == 200.0 / 255.0 && pats[1].color_b[2] == 200.0 / 255.0, "bound of faces 0..3: %g", pats[0].color_a[0]);
        CHECK(pats[3].color_a[1] == 90.0 / 255.0, "bound of the 1 x 1 faces over a darker own texture: %g", pats[3].color_a[1]);
        // two value-equal shapes under the two equal cube maps: one class
        std::vector<rt_material_desc> mats(2);
        std::memset(mats.data(), 0, 2 * sizeof mats[0]);
        mats[0].pattern = 0, mats[1].pattern = 1;
        std::vector<rt_shape_desc> s(2);
        std::memset(s.data(), 0, 2 * sizeof s[0]);
        for (auto& d : s) {
            d.kind = RT_SHAPE_CUBE;
            for (int i = 0; i < 16; ++i) d.inverse[i] = i % 5 == 0 ? 1.0 : 0.0;
        }
        s[1].material = 1;
        std::vector<uint32_t> cls;
        CHECK(ident::shape_classes(s.data(), 2, mats.data(), pats.data(), cls) == 1 && cls[1] == 0, "equal cube maps: one class");
        mats[1].pattern = 2;
        CHECK(ident::shape_classes(s.data(), 2, mats.data(), pats.data(), cls) == 0, "a differing face: two classes");
        std::printf("cube maps: by their faces' pictures\n");
    }

    // ---- 4: without a map list the renumbering is what it was
    {
        std::vector<rt_pattern_desc> a = {pattern(RT_PATTERN_IMAGE, 1, 0), pattern(RT_PATTERN_IMAGE, 2, 1)}, b = a;
        inst::canonical_image_patterns(a.data(), 2, tex, 4);
        std::vector<int32_t> records;
        inst::canonical_image_patterns(b.data(), 2, tex, 4, nullptr, 0, &records);
        CHECK(std::memcmp(a.data(), b.data(), 2 * sizeof a[0]) == 0 && a[0].sub_a == 0 && a[1].sub_a == 2 && a[1].reserved == 1, "unchanged");
        std::printf("no maps: the renumbering of textures alone\n");
    }

    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
