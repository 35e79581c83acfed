// chunk_spans.cpp -- the span arithmetic and the carry-slot rule of the chunked entries (rust_ray_tracing_amd/csrc/chunk_paths.h)
// under AddressSanitizer + UBSan on the CPU, without HIP and without libmipt.so.  Every (chunk size 1 ... 9, samples 1 ... 20, items
// 1 ... 12) is walked chunk after chunk as mipt::chunked_trace walks a call, and a brute force over the paths checks what the fold
// kernels rely on; the carry is played through two slots that hold an item and how many of its paths have been added.  Then the
// largest operands: first_path + n_paths = 2^63 - 1 and samples = 2^32 - 1, against 128-bit arithmetic.
// Built and run by tests/test_cpp_host.py::test_chunk_spans_under_asan_ubsan.
#include "../../rust_ray_tracing_amd/csrc/chunk_paths.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

using namespace mipt;
typedef unsigned long long u64;

u64 g_chunk, g_samples, g_items, g_index;                // the case a failure names
#define CHECK(cond)                                                                                                     \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            fprintf(stderr, "chunk_spans: line %d: %s (chunk size %llu, samples %llu, items %llu, chunk %llu)\n", __LINE__, #cond, g_chunk, \
                    g_samples, g_items, g_index);                                                                      \
            exit(1);                                                                                                   \
        }                                                                                                              \
    } while (0)

const u64 kNobody = ~0ull;
struct Slot { u64 item, added; };

void walk(u64 cap, unsigned samples, u64 n_items) {
    g_chunk = cap; g_samples = samples; g_items = n_items;
    const u64 total = n_items * samples, chunk = total < cap ? total : cap;
    std::vector<unsigned> covered(total, 0u);
    std::vector<u64> added(n_items, 0ull);               // paths of the item folded so far: its next span starts there
    Slot slot[2] = {{kNobody, 0}, {kNobody, 0}};
    u64 carried_out_before = kNobody;                    // the item the chunk before left in its out slot
    unsigned out_before = 2;
    g_index = 0;
    for (u64 first = 0; first < total; first += chunk, g_index++) {
        const u64 n_paths = total - first < chunk ? total - first : chunk;
        // the items with a path in the chunk, by brute force
        u64 lo = kNobody, hi = 0;
        for (u64 q = first; q < first + n_paths; q++) { const u64 p = q / samples; if (lo == kNobody) lo = p; hi = p; }
        const ChunkItems items = chunk_items(first, n_paths, samples);
        CHECK(items.p_first == lo && items.count == hi - lo + 1);
        const CarrySlots slots = carry_slots(g_index);
        CHECK(slots.in < 2 && slots.out < 2 && slots.in != slots.out);
        CHECK(g_index == 0 || slots.in == out_before);                                   // reads what the chunk before wrote
        u64 goes_on = kNobody, carried_out = kNobody;
        std::vector<ItemSpan> spans;
        for (u64 j = 0; j < items.count; j++) {
            const u64 p = items.p_first + j;
            const ItemSpan sp = item_span(first, n_paths, samples, p);
            CHECK(sp.begin == p * samples && sp.end == sp.begin + samples);
            CHECK(sp.q0 < sp.q1 && sp.q0 >= first && sp.q1 <= first + n_paths && sp.q0 >= sp.begin && sp.q1 <= sp.end);
            CHECK(sp.q0 == sp.begin + added[p]);                                          // contiguous and in order
            for (u64 q = sp.q0; q < sp.q1; q++) { CHECK(q / samples == p); covered[q]++; }
            if (sp.q0 != sp.begin) { CHECK(goes_on == kNobody && j == 0); goes_on = p; }
            if (sp.q1 != sp.end) { CHECK(carried_out == kNobody && j == items.count - 1); carried_out = p; }
            spans.push_back(sp);
        }
        CHECK(goes_on == carried_out_before);                                             // exactly the item left behind goes on
        // the lanes of a launch run in any order: play the worst one, the writer first
        if (carried_out != kNobody) {
            const ItemSpan &sp = spans.back();
            const u64 before = sp.q0 != sp.begin ? slot[slots.in].added : 0;
            if (sp.q0 != sp.begin) CHECK(slot[slots.in].item == carried_out && before == sp.q0 - sp.begin);
            slot[slots.out] = Slot{carried_out, before + (sp.q1 - sp.q0)};
        }
        for (u64 j = 0; j < items.count; j++) {
            const u64 p = items.p_first + j;
            const ItemSpan &sp = spans[j];
            if (sp.q0 != sp.begin) CHECK(slot[slots.in].item == p && slot[slots.in].added == added[p]);
            added[p] += sp.q1 - sp.q0;
            if (sp.q1 == sp.end) CHECK(added[p] == samples && p != carried_out);         // finished here: not the one carried out
            else CHECK(slot[slots.out].item == p && slot[slots.out].added == added[p]);
        }
        carried_out_before = carried_out;
        out_before = slots.out;
    }
    CHECK(carried_out_before == kNobody);
    for (u64 q = 0; q < total; q++) CHECK(covered[q] == 1u);
    for (u64 p = 0; p < n_items; p++) CHECK(added[p] == samples);
}

void edges() {
    g_chunk = g_samples = g_items = g_index = 0;
    typedef unsigned __int128 u128;
    const unsigned samples = 0xffffffffu;
    const u64 last = (1ull << 63) - 1ull, n_paths = 1ull << 22, first = last - n_paths;
    const ChunkItems items = chunk_items(first, n_paths, samples);
    const u128 p_first = (u128)first / samples, p_last = ((u128)first + n_paths - 1) / samples;
    CHECK((u128)items.p_first == p_first && (u128)items.count == p_last - p_first + 1 && items.count == 1);
    const ItemSpan sp = item_span(first, n_paths, samples, items.p_first);
    CHECK((u128)sp.begin == p_first * samples && (u128)sp.end == p_first * samples + samples);
    CHECK(sp.begin < first && sp.q0 == first && sp.end > sp.begin);                      // no wrap: the end lies above the beginning
    CHECK(sp.q1 == (sp.end < last ? sp.end : last) && sp.q1 > sp.q0);
    // the last item of the largest call: n = 2^31 - 1 items of 2^32 - 1 samples, its last chunk
    const u64 total = ((1ull << 31) - 1ull) * samples, tail = total % n_paths ? total % n_paths : n_paths;
    const ChunkItems end_items = chunk_items(total - tail, tail, samples);
    CHECK(end_items.p_first + end_items.count == (1ull << 31) - 1ull);
    const ItemSpan end_sp = item_span(total - tail, tail, samples, (1ull << 31) - 2ull);
    CHECK(end_sp.end == total && end_sp.q1 == total && end_sp.q0 == total - tail && end_sp.begin < end_sp.q0);
}

} // namespace

int main() {
    for (u64 cap = 1; cap <= 9; cap++)
        for (unsigned samples = 1; samples <= 20; samples++)
            for (u64 n_items = 1; n_items <= 12; n_items++) walk(cap, samples, n_items);
    edges();
    printf("chunk_spans ok\n");
    return 0;
}
