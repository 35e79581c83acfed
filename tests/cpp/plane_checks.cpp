// plane_checks.cpp -- the device-free checks of the image-space entries (rust_ray_tracing_amd/csrc/mipt_planes.h) under
// AddressSanitizer + UBSan on the CPU, without HIP and without libmipt.so: plane sets of zero, one and kMaxPlanes planes, absent
// optional planes, ranges that touch or share one byte, the one allowed alias, ranges at the top of the address space, and
// inverse_square at the edges of f32.  Every result is held to a value written here.
// Built and run by tests/test_cpp_host.py::test_plane_checks_under_asan_ubsan.
#include "../../rust_ray_tracing_amd/csrc/mipt_planes.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

namespace {
std::string g_error;                                     // the text mipt::fail last set
}
void mipt_internal_set_error(const char *msg) { g_error = msg; }

namespace {

using namespace mipt;

#define CHECK(cond)                                                                                                     \
    do {                                                                                                               \
        if (!(cond)) { fprintf(stderr, "plane_checks: line %d: %s (last error: %s)\n", __LINE__, #cond, g_error.c_str()); exit(1); } \
    } while (0)

bool refused(int rc, const char *text) { return rc == MIPT_ERR_INVALID_ARG && g_error == text; }

// a buffers struct as include/mipt.h lays them out: the plane pointers, then reserved
struct Buffers { const void *plane[kMaxPlanes]; void *reserved[3]; };

const void *at(uintptr_t a) { return (const void *)a; }

} // namespace

int main() {
    static Plane table[kMaxPlanes];
    static char names[kMaxPlanes][4];
    for (int i = 0; i < kMaxPlanes; i++) {
        snprintf(names[i], sizeof names[i], "p%d", i);
        table[i] = Plane{names[i], 4, 4, false, kPlaneIn, -1};
    }
    const uint64_t n_pix = 64, bytes = n_pix * 4;
    PlaneSet set;

    {   // no plane at all: nothing to miss, nothing to overlap
        Buffers b{};
        planes_bind(set, table, 0, &b);
        planes_size(set, n_pix);
        CHECK(planes_required("e", set) == MIPT_OK && planes_disjoint("e", set) == MIPT_OK);
    }
    {   // one plane: required and absent, then present
        Buffers b{};
        table[0].required = true;
        planes_bind(set, table, 1, &b);
        planes_size(set, n_pix);
        CHECK(refused(planes_required("e", set), "e: null p0"));
        b.plane[0] = at(0x1000);
        planes_bind(set, table, 1, &b);
        CHECK(planes_required("e", set) == MIPT_OK && planes_disjoint("e", set) == MIPT_OK && set.bytes[0] == bytes);
    }
    {   // the most planes a set holds, end to start: each range touches the next and none overlaps
        Buffers b{};
        for (int i = 0; i < kMaxPlanes; i++) b.plane[i] = at(0x10000 + (uintptr_t)i * bytes);
        planes_bind(set, table, kMaxPlanes, &b);
        planes_size(set, n_pix);
        CHECK(planes_required("e", set) == MIPT_OK && planes_disjoint("e", set) == MIPT_OK);
        // the last one a byte lower: it shares exactly one byte with the one before it
        set.ptr[kMaxPlanes - 1] = at(0x10000 + (uintptr_t)(kMaxPlanes - 1) * bytes - 1);
        CHECK(refused(planes_disjoint("e", set), "e: p11 overlaps p10"));
        // the pair found first is the one reported: lowest i, then lowest j
        set.ptr[3] = set.ptr[1];
        CHECK(refused(planes_disjoint("e", set), "e: p3 overlaps p1"));
        // an absent optional plane overlaps nothing and is not missed, wherever the others are
        set.ptr[3] = nullptr; set.ptr[kMaxPlanes - 1] = nullptr;
        CHECK(planes_required("e", set) == MIPT_OK && planes_disjoint("e", set) == MIPT_OK);
        // a required one among them is
        table[7].required = true;
        set.ptr[7] = nullptr;
        CHECK(refused(planes_required("e", set), "e: null p7"));
        table[7].required = false;
    }
    {   // the allowed alias: an output given as exactly the input it may go over; four bytes off it is an overlap like any other
        Buffers b{};
        b.plane[0] = at(0x1000); b.plane[1] = at(0x8000); b.plane[2] = at(0x1000);
        table[2].use = kPlaneOut; table[2].over = 0;
        planes_bind(set, table, 3, &b);
        planes_size(set, n_pix);
        CHECK(planes_disjoint("e", set) == MIPT_OK);
        set.ptr[2] = at(0x1004);
        CHECK(refused(planes_disjoint("e", set), "e: p2 overlaps p0 (only p2 == p0 is allowed)"));
        set.ptr[2] = at(0x1000 - 4);
        CHECK(refused(planes_disjoint("e", set), "e: p2 overlaps p0 (only p2 == p0 is allowed)"));
        // the alias is that pair's alone: the same address for another pair is refused, with the table's one exception named
        set.ptr[2] = at(0x20000); set.ptr[1] = at(0x1000);
        CHECK(refused(planes_disjoint("e", set), "e: p1 overlaps p0 (only p2 == p0 is allowed)"));
        table[2].use = kPlaneIn; table[2].over = -1;
    }
    {   // ranges_overlap itself
        CHECK(!ranges_overlap(at(0x1000), 16, at(0x1010), 16) && !ranges_overlap(at(0x1010), 16, at(0x1000), 16));   // touching
        CHECK(ranges_overlap(at(0x1000), 17, at(0x1010), 16) && ranges_overlap(at(0x1010), 16, at(0x1000), 17));     // one byte
        CHECK(ranges_overlap(at(0x1000), 16, at(0x1000), 16) && ranges_overlap(at(0x1000), 64, at(0x1010), 4));
        CHECK(!ranges_overlap(at(0x1000), 0, at(0x1000), 16));                                                         // an empty range
        // at the top of the address space the ends a + bytes wrap to small numbers.  A range that ends exactly at the top wraps to 0,
        // and nothing is below 0: it is reported apart from everything, itself included
        const uintptr_t top = std::numeric_limits<uintptr_t>::max();
        CHECK(!ranges_overlap(at(top - 15), 16, at(top - 15), 16));
        CHECK(!ranges_overlap(at(top - 31), 32, at(top - 15), 16) && !ranges_overlap(at(top - 15), 16, at(top - 31), 32));
        // one that ends a byte short of the top does not wrap and is compared as usual
        CHECK(ranges_overlap(at(top - 16), 16, at(top - 16), 16) && !ranges_overlap(at(top - 32), 16, at(top - 16), 16));
        // a wrapped range against a low one: only "low start below the wrapped end" is left of the test
        CHECK(!ranges_overlap(at(top - 15), 32, at(0x1000), 16) && !ranges_overlap(at(0x1000), 16, at(top - 15), 32));
    }
    {   // alignment: the plane's own, 4 for words and 16 for the histories; an absent plane is aligned
        Buffers b{};
        b.plane[0] = at(0x1002); b.plane[1] = at(0x1008); b.plane[2] = at(0x1010);
        table[1].align = table[2].align = 16;
        planes_bind(set, table, 4, &b);
        CHECK(refused(plane_aligned("e", set, 0), "e: p0 must be 4-byte aligned"));
        CHECK(refused(plane_aligned("e", set, 1), "e: p1 must be 16-byte aligned"));
        CHECK(plane_aligned("e", set, 2) == MIPT_OK && plane_aligned("e", set, 3) == MIPT_OK);
        table[1].align = table[2].align = 4;
    }
    {   // the frame
        uint64_t n = 1;
        CHECK(refused(not_null("e", nullptr, "opt"), "e: null opt") && not_null("e", &n, "opt") == MIPT_OK);
        CHECK(refused(frame_nonzero("e", 0, 4, 2), "e: width and height must be greater than 0"));
        CHECK(refused(frame_nonzero("e", 8, 0, 0), "e: width and height must be greater than 0"));
        CHECK(refused(frame_nonzero("e", 8, 4, 0), "e: n_views == 0") && frame_nonzero("e", 8, 4, 2) == MIPT_OK);
        CHECK(frame_pixels("e", 8, 4, 2, &n) == MIPT_OK && n == 64);
        CHECK(frame_pixels("e", 65535, 65537, 1, &n) == MIPT_OK && n == 4294967295ull);
        CHECK(refused(frame_pixels("e", 65536, 65536, 1, &n), "e: 1 views of 65536x65536: n_views*width*height must stay below 2^32") && n == 0);
        CHECK(refused(frame_pixels("e", 4294967295u, 4294967295u, 4294967295u, &n),
                      "e: 4294967295 views of 4294967295x4294967295: n_views*width*height must stay below 2^32"));
        CHECK(flags_zero("e", 0) == MIPT_OK && refused(flags_zero("e", 0x80000000u), "e: flags 0x80000000: must be 0"));
        uint32_t words[8] = {};
        Buffers b{};
        CHECK(reserved_zero("e", words, b.reserved) == MIPT_OK);
        b.reserved[2] = &n;
        CHECK(refused(reserved_zero("e", words, b.reserved), "e: reserved buffer pointers must be NULL"));
        words[7] = 1;
        CHECK(refused(reserved_zero("e", words, b.reserved), "e: reserved option fields must be 0"));
        CHECK(tiles_across(1) == 1 && tiles_across(64) == 1 && tiles_across(65) == 2 && tiles_across(1920) == 30);
        CHECK(tiles_down(1) == 1 && tiles_down(4) == 1 && tiles_down(9) == 3 && tiles_down(1080) == 270);
    }
    {   // inverse_square: 1 / sigma^2 in f32, refused unless sigma and the result are finite and greater than 0
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        float k = -1.0f;
        CHECK(!inverse_square(0.0f, &k) && !inverse_square(-0.0f, &k) && !inverse_square(-2.0f, &k) && k == -1.0f);
        CHECK(!inverse_square(inf, &k) && !inverse_square(-inf, &k) && !inverse_square(nan, &k) && k == -1.0f);
        CHECK(!inverse_square(1e-20f, &k) && std::isinf(k));             // sigma^2 = 1e-40 is subnormal, its inverse beyond f32
        CHECK(!inverse_square(1e20f, &k) && k == 0.0f);                  // sigma^2 is +inf
        CHECK(inverse_square(0.5f, &k) && k == 4.0f);
        CHECK(inverse_square(4.0f, &k) && k == 0.0625f);
    }
    printf("plane_checks ok\n");
    return 0;
}
