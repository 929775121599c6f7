// sha1_kernels.h -- kernel arguments and launchers (internal to libsha1chunk).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// One batch of independent messages.  Message e (0 <= e < n) is chunk
// id = order ? order[e] : e, bytes base[off[id] .. off[id] + len[id]),
// with off/len replaced by id*ulen / ulen when the arrays are null.
struct BatchArgs {
    const uint8_t* base;
    const uint64_t* off;
    const uint32_t* len;
    uint32_t ulen;
    uint32_t n;
    const uint32_t* order;
    uint8_t* dig;  // n x 20 digest bytes (finalising mode), 4-byte aligned
    // Streaming extras (null/0 for plain batches).  init_state/out_state:
    // every kernel; prefix_bytes (finalising a stream): lane kernel only.
    const uint32_t* init_state;  // 5 words per message instead of the IV
    uint64_t prefix_bytes;       // bytes already hashed before this call
    uint32_t* out_state;         // non-null: no padding, write raw state
    // Mixed-batch kernel only: its device-side plan {mode, H, F}
    // (plan_mixed_kernel, sha1_kernels.hip).
    const uint32_t* plan;
};

// Launch counters (diagnostics: s1be_launch_stats, rt_device.hip; read by
// tests/launch_stats.py).  One per distinct thing the library can launch,
// process-wide, counted by the launcher where it enqueues the kernels (after
// its n == 0 return), not where the shape is chosen.  The layout of
// s1be_launch_stats' out[12] is this enum's order:
//   [0] lane  [1] fused  [2] split unit 1  [3] split unit 4
//   [4] split unit 11, lane-per-chunk loads  [5] split unit 11, shared loads
//   [6] quad (unit 416)  [7] a study shape (A/B library)  [8] mixed
//   [9] length sort  [10] persistent verify-queue drain
//   [11] gauge, never reset: CUs the calling thread's device's drains hold
enum LaunchCounter {
    kLaunchLane, kLaunchFused, kLaunchSplit1, kLaunchSplit4, kLaunchSplit11Lane, kLaunchSplit11Shared,
    kLaunchQuad, kLaunchStudy, kLaunchMixed, kLaunchSort, kLaunchDrain, kLaunchCounters
};
void count_launch(LaunchCounter which);

hipError_t launch_lane(const BatchArgs& A, hipStream_t st);
hipError_t launch_fused(const BatchArgs& A, hipStream_t st);
// Split-kernel shapes (sha1_kernels.hip launch_split): 1 (1-block units), 4
// (4-block units, two producers: <= 1 group per CU), 11 (8-wave workgroup of
// two pairs: <= 2 groups per CU), kSplitUnitQuad (4-block units, two
// producers, a quad of lanes per chunk and 16 chunks per workgroup: <= 16
// chunks per CU; sha1_split.hpp kVQuad).  The A/B library (`make ab`,
// -DSHA1CHUNK_AB_VARIANTS) also builds the study's other shapes and variant
// flags (2, 3, 8-10, 12, 13, 10*U+V, 500+V, 569, 577-585, 86, 87, 590; 417:
// the quad shape with the consumer's cycle probe; 816 / 817: the quad shape
// with 8-block units, which lost to 4, profiles/quad_unit_probe.json).
constexpr int kSplitUnitQuad = 416;
bool split_unit_built(int unit_blocks);
hipError_t launch_split(const BatchArgs& A, int unit_blocks, hipStream_t st);
// The other shapes of the split-kernel study: weak stubs in the product
// (no such shape), defined by tools/ab_kernels.hip in the A/B library.
bool split_unit_study_built(int unit_blocks);
hipError_t launch_split_study(const BatchArgs& A, int unit_blocks, hipStream_t st);
// Sorted ragged batch of more groups than CUs (A.order set, sorted_len =
// the lengths in that order): a device-side plan splits the groups between
// the one-group split shape (longest first) and the fused kernel, or runs
// them all in the 8-wave split shape (sha1_kernels.hip, mixed).  `plan`:
// 3 device words; forced (or null): {mode, H, F} instead of the planner's.
uint32_t mixed_grid(uint32_t groups, int cus, uint32_t* hcap);
// Exact order of the chunks whose 16-bit sort keys clamp (>= 65535 SHA-1
// blocks: 4 MiB and more).  The sort leaves them at the front in caller
// order; the mixed path's layout kernel re-ranks up to kBigExact of them by
// their exact block counts (stable) before the planner and the hash kernel
// read the order (sha1_kernels.hip plan_layout_kernel).  More than that
// keep caller order among themselves (digests unaffected).
constexpr uint32_t kBigExact = 4096;
struct BigFix {
    const uint32_t* cnt;   // per sort tile: its chunks whose key clamped (sort_hist<1>)
    uint32_t tiles;
    const uint32_t* len;   // positions [0, min(m, kBigExact)) of the sort's output:
    const uint32_t* id;    //   their lengths and chunk ids (sort_scatter<2>)
    uint32_t* order;       // the sort's order and (group-head) sorted lengths,
    uint32_t* sorted_len;  //   rewritten for positions < m
};
// big (or null: no re-ranking): the sort's BigFix.
hipError_t launch_mixed(const BatchArgs& A, const uint32_t* sorted_len, const BigFix* big, uint32_t* plan, int cus,
                        const int* forced, hipStream_t st);
// The layout summary alone (its re-ranking included): the diagnostics of
// s1be_mixed_order_async.
hipError_t launch_plan_layout(const BatchArgs& A, const uint32_t* sorted_len, const BigFix* big, uint32_t* plan,
                              hipStream_t st);
// Persistent verify-queue drain (sha1_kernels.hip, vq drain; host side in
// vq_persistent.hip, the persistent sha1chunk_vq).  The queue's rings live in
// coherent pinned host memory, which the kernel reads over PCIe (no copy
// engine, no launch per batch); results go back to host memory.
struct VqDrainArgs {
    const uint8_t* data;     // host: chunk bytes (ring)
    const uint64_t* off;     // host: per slot, byte offset into data
    const uint32_t* len;     // host: per slot, chunk length
    const uint8_t* exp;      // host: per slot, expected digest (20 B)
    const uint32_t* grp;     // host: per group ring entry {first slot, count}
    const uint32_t* pub;     // host: groups published so far
    const uint32_t* stop;    // host: nonzero = exit once nothing is claimable
    uint8_t* alive;          // host: per workgroup, 1 while it may still claim
    uint8_t* res;            // host: per slot, 0 match / 1 mismatch
    uint32_t* done;          // host: per group ring entry, group index + 1 when done
    uint32_t* last_done;     // host: the last group finished (index + 1), any order
    uint8_t* dig;            // device: per slot, digest scratch
    uint32_t* claim;         // device: groups claimed so far
    uint32_t grp_ring;       // group ring entries
    uint32_t pad;
    uint64_t idle_ticks;     // 100 MHz ticks without work before a workgroup exits
    uint64_t life_ticks;     // 100 MHz ticks after which a workgroup exits even under load
};
hipError_t launch_vq_drain(const VqDrainArgs& Q, uint32_t grid, hipStream_t st);

// Progressive verify (sha1_progress.hip; host side in sha1_pv.hip, the
// sha1chunk_pv object).  One launch advances any number of receive sessions:
// work-list entry e says which bytes of its session became final since the
// session's last entry, and lane e hashes exactly those.  The session
// buffers, the work list, the expected digests and the results live in
// pinned host memory (read and written over PCIe); only the midstates are in
// device memory.
struct PvEntry {
    uint32_t session;  // index of the session (buffer at data + session * stride)
    uint32_t from;     // bytes hashed by the session's earlier entries, a multiple of 64
    uint32_t upto;     // final bytes: a multiple of 64, or len when `final`
    uint32_t len;      // the chunk's length
    uint32_t final;    // nonzero: upto == len; pad, compare, publish
    uint32_t gen;      // the session's generation, published in done[session]
    uint32_t pad[2];   // 32 bytes: two 16-byte loads per lane
};
struct PvArgs {
    const uint8_t* data;       // host: sessions x stride bytes, 128-byte aligned buffers
    uint64_t stride;
    const PvEntry* work;       // host: n entries, at most one per session
    uint32_t n;
    uint32_t sessions;
    uint32_t* state;           // device: 5 midstate words per session
    const uint32_t* expected;  // host: 8 words per session, the first 5 the expected digest
    uint32_t* result;          // host: 8 words per session: digest (5), mismatch (1)
    uint32_t* done;            // host: per session, its generation once the result is written
    const uint8_t* dummy;      // device: 64 bytes no session owns (shared kernel: a slot with nothing to load)
};
// depth: 64-byte blocks of each lane in flight ahead of its compression (2, 4 or 8).
hipError_t launch_progress(const PvArgs& P, int depth, hipStream_t st);
// The same work with the bulk blocks' loads shared across the wave, four
// lanes per entry (sha1_progress_shared.hip): for many sessions at once.
hipError_t launch_progress_shared(const PvArgs& P, hipStream_t st);

// Batched SHA1Init / SHA1Update / SHA1Final over an array of 96-byte
// SHA1Context structs in device memory (sha1_update.hip; host side in
// rt_update.hip).  Entry i works on context index ? index[i] : i; an entry
// whose context index is >= n_contexts, or whose context says more than 63
// staged bytes, is skipped by every kernel.
struct UpdateArgs {
    uint8_t* ctx;           // n_contexts structs of 96 bytes, 8-byte aligned
    uint64_t n_contexts;
    const uint32_t* index;  // n context indices, or null: entry i is context i
    uint32_t n;
    // update only: entry i's piece is base[off[i] .. off[i] + len[i])
    const uint8_t* base;
    const uint64_t* off;
    const uint32_t* len;
    // update scratch, n entries each: the piece's whole-block span after the
    // head (what the bulk launch hashes) and the packed chaining values
    // (BatchArgs::init_state / out_state of that launch, in place)
    uint64_t* mid_off;
    uint32_t* mid_len;
    uint32_t* state;
    uint8_t* dig;  // final only: n x 20 digest bytes, 4-byte aligned, or null
};
hipError_t launch_update_init(const UpdateArgs& U, hipStream_t st);
hipError_t launch_update_pre(const UpdateArgs& U, hipStream_t st);
hipError_t launch_update_post(const UpdateArgs& U, hipStream_t st);
hipError_t launch_update_final(const UpdateArgs& U, hipStream_t st);

// Reassembly of messages given as segment lists (sha1_gather.hip; host side in
// rt_gather.hip).  Message i is segments seg_first[i] .. seg_first[i+1]-1,
// segment s being seg_len[s] bytes at base + seg_off[s]; it is written
// contiguously at dst + dst_off[i], or skipped (gather_map.hpp skip_range,
// skip_total): then no byte is written and its length word is 0xFFFFFFFF.
// n and n_segments are at most 2^32 - 1025.
struct GatherArgs {
    const uint8_t* base;
    const uint64_t* seg_off;
    const uint32_t* seg_len;
    uint64_t n_segments;
    const uint32_t* seg_first;  // n + 1 entries
    uint32_t n;
    uint8_t* dst;
    const uint64_t* dst_off;
    uint64_t dst_bytes;
    uint32_t* out_len;  // n length words for the caller, or null
    // scratch: each segment's position inside its message (n_segments
    // entries) and each message's length word (n entries)
    uint32_t* pos;
    uint32_t* mlen;
    uint32_t* skipped;  // one device counter: messages skipped, added up
};
hipError_t launch_gather_scan(const GatherArgs& G, hipStream_t st);
hipError_t launch_gather_copy(const GatherArgs& G, hipStream_t st);

// The digest index (sha1_index.hip, arithmetic in index_map.hpp; host side in
// rt_index.hip): an open-addressed array of `mask + 1` position words over a
// table of m digests of five words each.
struct IndexArgs {
    const uint32_t* table;  // m x 5 words, read only
    uint32_t m;             // at most 2^31
    uint32_t* slots;        // mask + 1 words; 0xFFFFFFFF = empty
    uint32_t mask;
    // the build's counters, zeroed before it: the longest probe in slots
    // visited, entries whose digest was in place already, entries whose probe
    // wrapped past the last slot
    unsigned long long* stats;
};
// One lane per table entry; the slots hold 0xFFFFFFFF and the counters 0.
hipError_t launch_index_build(const IndexArgs& X, hipStream_t st);
// One lane per query of five words: ids[i] = the lowest position of
// queries[5i .. 5i+4] in the table, or 0xFFFFFFFF (n at most 2^32 - 256).
// Only after the build is complete.
hipError_t launch_index_lookup(const IndexArgs& X, const uint32_t* queries, uint32_t n, uint32_t* ids,
                               hipStream_t st);

// One lane per appended entry: table row base + i, i < k, is inserted unless
// skip (k bytes, or null) says skip[i] != 0.  The rows were written by an
// earlier operation on the stream; base + k <= 2^31; X.stats points at the
// counters this launch adds to (the build's three, in the same order).
hipError_t launch_index_append(const IndexArgs& X, uint32_t base, uint32_t k, const uint8_t* skip, hipStream_t st);
// Growth: one lane per slot of a finished array of old_mask + 1 words; what it
// holds is inserted into X.slots (emptied before) over X.table, which holds
// every row the old table held.  Counts nothing.
hipError_t launch_index_rehash(const IndexArgs& X, const uint32_t* old_slots, uint32_t old_mask, hipStream_t st);

// One workgroup of kSynthThreads per chunk.  A launch holds fewer than 2^32
// work-items per dimension (the dispatch packet's grid size is a 32-bit count
// of work-items), so one call fills at most kSynthMaxChunks chunks; a larger
// count is hipErrorInvalidValue (the C ABI refuses it before it gets here).
constexpr uint32_t kSynthThreads = 256;
constexpr uint64_t kSynthMaxChunks = 0xffffffffull / kSynthThreads;  // 2^24 - 1
hipError_t launch_synth(uint8_t* dst, const uint64_t* off, const uint32_t* lens, uint32_t ulen,
                        uint64_t first, uint64_t count, uint64_t seed, hipStream_t st);
hipError_t launch_compare(const uint8_t* dig, const uint8_t* exp, uint32_t n, uint8_t* mismatch,
                          hipStream_t st);

// Longest-first order of a ragged batch (sha1_sort.hip): *d_order receives n
// indices in descending order of SHA-1 block count (stable), *d_sorted_len
// the lengths in that order at each group's first position (64g; the
// planner reads no other) and *d_plan the mixed kernel's plan area of the
// same allocation
// (mixed_plan_bytes(n): 256 bytes of plan words, then the planner's layout
// summary); release *scratch with hipFreeAsync on the same stream after the
// consuming kernel has been enqueued.
inline size_t mixed_plan_bytes(uint32_t n) {
    const size_t words = ((size_t(n) + 63) / 64 + 31) / 32;  // one per 32 groups of 64 chunks
    return 256 + ((words * 12 + words * 32 * 4 + 255) & ~size_t(255));  // + a block count per group
}
// big (or null): receives the clamped chunks' re-ranking inputs (BigFix).
hipError_t sort_by_length_desc(const uint32_t* d_len, uint32_t n, const uint32_t** d_order,
                               const uint32_t** d_sorted_len, uint32_t** d_plan, void** scratch, BigFix* big,
                               hipStream_t st);
// out[i] = len[order[i]] for every i (diagnostics: s1be_sort_order_async).
hipError_t gather_sorted_lengths(const uint32_t* d_len, const uint32_t* d_order, uint32_t* d_out, uint32_t n,
                                 hipStream_t st);
