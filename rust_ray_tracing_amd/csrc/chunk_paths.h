// chunk_paths.h -- the arithmetic of the entries that trace n items x samples paths in chunks (mipt::chunked_trace, mipt_scene.h; the
// kernels: bake.hip, probe.hip).  Paths are numbered item after item; a chunk is paths [first_path, first_path + n_paths), n_paths > 0.
// Plain integers and no HIP type, so that tests/cpp/chunk_spans.cpp builds it with the host compiler; constexpr, which under hipcc
// makes a function host and device code.  first_path + n_paths < 2^63 and 0 < samples < 2^32: nothing wraps but path_rng, which is
// meant to.
#pragma once

namespace mipt {

// the grid of a grid-stride kernel with blocks of `block` lanes: a block per `block` work items, at most 8 per CU, at least 1
constexpr unsigned grid_for(unsigned long long work, int n_cu, unsigned block) {
    const unsigned long long blocks = (work + block - 1) / block, cap = (unsigned long long)(n_cu > 0 ? n_cu : 1) * 8ull;
    return (unsigned)(blocks > cap ? cap : blocks < 1 ? 1 : blocks);
}

// path j of the chunk: path q of the call, sample s of item p (include/mipt.h "the sample")
struct PathOf { unsigned long long q, p; unsigned s; };
constexpr PathOf path_of(unsigned long long first_path, unsigned samples, unsigned long long j) {
    const unsigned long long q = first_path + j, p = q / samples;
    return PathOf{q, p, (unsigned)(q - p * samples)};
}
// the stream of sample s of the item whose seed is seed_word: cpu.rs:28-29 with the item as the pixel and the sample as the frame,
// wrapping, 1 in place of 0
constexpr unsigned path_rng(unsigned seed_word, unsigned first_sample, unsigned sample_stride, unsigned s) {
    const unsigned rng = 987612486u * (seed_word + (first_sample + s) * sample_stride + 87636354u);
    return rng == 0u ? 1u : rng;
}

struct ChunkItems { unsigned long long p_first, count; };        // items [p_first, p_first + count) have a path in the chunk
constexpr ChunkItems chunk_items(unsigned long long first_path, unsigned long long n_paths, unsigned samples) {
    const unsigned long long p_first = first_path / samples, p_last = (first_path + n_paths - 1ull) / samples;
    return ChunkItems{p_first, p_last - p_first + 1ull};
}
// Item p's paths are [begin, end); those of them in the chunk are [q0, q1), not empty for an item of chunk_items.  q0 != begin: its
// samples began in a chunk before, and it goes on from carry_in.  q1 != end: they go on behind this chunk, and it leaves its sums in
// carry_out.  A chunk has at most one item of each kind -- its first and its last, the same one where the chunk lies inside an item.
struct ItemSpan { unsigned long long begin, end, q0, q1; };
constexpr ItemSpan item_span(unsigned long long first_path, unsigned long long n_paths, unsigned samples, unsigned long long p) {
    const unsigned long long last_path = first_path + n_paths;   // one past
    const unsigned long long begin = p * samples, end = begin + samples;
    return ItemSpan{begin, end, begin > first_path ? begin : first_path, end < last_path ? end : last_path};
}
// The two carry slots, chunks numbered from 0: a chunk leaves its last item's sums in slot `out` and takes its first item's from slot
// `in`, which the chunk before wrote.  Never the same slot: the two items are different lanes of one launch.
struct CarrySlots { unsigned in, out; };
constexpr CarrySlots carry_slots(unsigned long long chunk_index) { return CarrySlots{(unsigned)(~chunk_index & 1ull), (unsigned)(chunk_index & 1ull)}; }

} // namespace mipt
