// owned_guard.cpp -- mipt::Owned (mipt_internal.h) under AddressSanitizer + UBSan on the CPU: the owner every function of libmipt.so
// holds its device memory, streams and events in, here over a release function that only records what it is given.  And
// mipt::Grown, the grow-on-demand owner of a scene's workspace buffers, over an allocator and a release function that count.
// Built and run by tests/test_cpp_host.py::test_owned_guard_under_asan_ubsan.
#include "../../rust_ray_tracing_amd/csrc/mipt_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// mipt::Grown, the owner of a block that grows on demand (a scene's workspace), over malloc and free that count: ASan sees a block
// freed twice, used after its free or never freed
int g_allocs = 0, g_frees = 0;
bool g_alloc_fails = false;
int counting_alloc(void **p, size_t bytes) {
    if (g_alloc_fails) return 2;                         // like hipMalloc: a status, *p untouched
    g_allocs++;
    *p = malloc(bytes ? bytes : 1);
    return 0;
}
void counting_free(void *p) { g_frees++; free(p); }
using Block = mipt::Grown<char, counting_alloc, counting_free>;

bool counts_are(int allocs, int frees) { return g_allocs == allocs && g_frees == frees; }

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
    {   // Grown: from empty; a smaller or equal request keeps the block; a larger one frees it once, then allocates
        {
            Block b;
            CHECK(!b && b.get() == nullptr && b.bytes() == 0 && counts_are(0, 0));
            CHECK(b.grow(100) == 0 && b && b.bytes() == 100 && counts_are(1, 0));
            char *const first = b.get();
            memset(first, 0xAB, 100);
            CHECK(b.grow(100) == 0 && b.get() == first && b.bytes() == 100 && counts_are(1, 0));
            CHECK(b.grow(1) == 0 && b.get() == first && b.bytes() == 100 && counts_are(1, 0));
            CHECK(b.grow(0) == 0 && b.get() == first && b.bytes() == 100 && counts_are(1, 0));
            CHECK(b.grow(101) == 0 && b.bytes() == 101 && counts_are(2, 1));
            memset(b.get(), 0xCD, 101);
        }
        CHECK(counts_are(2, 2));                         // one release at scope end
    }
    {   // an allocation that fails leaves the owner empty with size 0, the old block freed once; the next grow starts over
        g_allocs = g_frees = 0;
        {
            Block b;
            CHECK(b.grow(64) == 0 && counts_are(1, 0));
            g_alloc_fails = true;
            CHECK(b.grow(32) == 0 && b.bytes() == 64 && counts_are(1, 0));       // large enough: the allocator is not asked
            CHECK(b.grow(65) == 2 && !b && b.get() == nullptr && b.bytes() == 0 && counts_are(1, 1));
            CHECK(b.grow(1) == 2 && !b && b.bytes() == 0 && counts_are(1, 1));
            g_alloc_fails = false;
            CHECK(b.grow(8) == 0 && b && b.bytes() == 8 && counts_are(2, 1));
            b.reset();
            b.reset();
            CHECK(!b && b.bytes() == 0 && counts_are(2, 2));
        }
        CHECK(counts_are(2, 2));                         // empty at scope end: nothing more
    }
    {   // a move takes block and size; the source is empty and releases nothing; move assignment frees what it overwrites
        g_allocs = g_frees = 0;
        {
            Block a;
            CHECK(a.grow(16) == 0);
            char *const p = a.get();
            Block b(std::move(a));
            CHECK(!a && a.bytes() == 0 && b.get() == p && b.bytes() == 16 && counts_are(1, 0));
            Block c;
            CHECK(c.grow(4) == 0 && counts_are(2, 0));
            c = std::move(b);
            CHECK(counts_are(2, 1) && c.get() == p && c.bytes() == 16 && !b && b.bytes() == 0);
            CHECK(a.grow(3) == 0 && a.bytes() == 3 && counts_are(3, 1));          // a moved-from owner grows again
        }
        CHECK(counts_are(3, 3));
    }
    {   // an owner of a pointer is cast like the bare pointer, to any pointer type, and still releases it once
        g_frees = 0;
        {
            mipt::Owned<char *, counting_free> p((char *)malloc(8));
            CHECK((const unsigned *)p == (const unsigned *)p.get() && (void *)p == (void *)p.get() && (char *)p == p.get());
        }
        CHECK(g_frees == 1);
    }
    printf("owned_guard ok\n");
    return 0;
}
