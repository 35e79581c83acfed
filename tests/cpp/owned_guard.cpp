// owned_guard.cpp -- mipt::Owned (mipt_internal.h) under AddressSanitizer + UBSan on the CPU: the owner every function of libmipt.so
// holds its device memory, streams and events in, here over a release function that only records what it is given.
// Built and run by tests/test_cpp_host.py::test_owned_guard_under_asan_ubsan.
#include "../../rust_ray_tracing_amd/csrc/mipt_internal.h"

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <utility>
#include <vector>

void mipt_internal_set_error(const char *) {}           // mipt::fail's sink (mipt_api.cpp in the library); unused here

namespace {

std::vector<int> g_freed;                                // the handles the fake was given, in order
int fake_free(int h) { g_freed.push_back(h); return 7; } // a status the owner must ignore
using Handle = mipt::Owned<int, fake_free>;

#define CHECK(cond)                                                                                                     \
    do {                                                                                                               \
        if (!(cond)) { fprintf(stderr, "owned_guard: line %d: %s\n", __LINE__, #cond); exit(1); }                      \
    } while (0)

bool freed_is(std::vector<int> want) {
    const bool same = g_freed == want;
    g_freed.clear();
    return same;
}

void three_in_a_scope(bool throws) {
    Handle a(1), b(2), c(3);
    if (throws) throw std::runtime_error("through the scope");
}

} // namespace

int main() {
    {   // a destructor releases its handle exactly once
        { Handle a(5); CHECK(a.get() == 5 && a); }
        CHECK(freed_is({5}));
    }
    {   // an empty or moved-from owner releases nothing
        { Handle e; CHECK(e.get() == 0 && !e); }
        CHECK(freed_is({}));
        {
            Handle a(6);
            Handle b(std::move(a));
            CHECK(a.get() == 0 && !a && b.get() == 6);
            CHECK(freed_is({}));
        }
        CHECK(freed_is({6}));
    }
    {   // move assignment releases the overwritten handle once and empties the source
        {
            Handle a(7), b(8);
            b = std::move(a);
            CHECK(freed_is({8}));
            CHECK(a.get() == 0 && b.get() == 7);
            Handle &self = b;
            b = std::move(self);                         // onto itself: nothing happens
            CHECK(freed_is({}) && b.get() == 7);
        }
        CHECK(freed_is({7}));
    }
    {   // release() hands the handle back and nothing is released afterwards
        int h;
        { Handle a(9); h = a.release(); CHECK(a.get() == 0); }
        CHECK(h == 9 && freed_is({}));
    }
    {   // reset() twice releases once; put() releases what was held and hands out the address of the empty slot
        {
            Handle a(10);
            a.reset();
            a.reset();
            CHECK(freed_is({10}));
            a.reset(11);
            *a.put() = 12;
            CHECK(freed_is({11}) && a.get() == 12);
        }
        CHECK(freed_is({12}));
    }
    {   // three owners in one scope are released in reverse order of declaration
        three_in_a_scope(false);
        CHECK(freed_is({3, 2, 1}));
    }
    {   // an exception thrown through that scope releases all three
        bool caught = false;
        try { three_in_a_scope(true); } catch (const std::runtime_error &) { caught = true; }
        CHECK(caught && freed_is({3, 2, 1}));
    }
    printf("owned_guard ok\n");
    return 0;
}
