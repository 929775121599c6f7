// pv_shared_map.hpp -- the address arithmetic of the shared loads of
// sha1_progress_shared_kernel (sha1_progress_shared.hip), as plain constexpr
// functions: the kernel includes it, and tools/pv_shared_map_check.cc checks
// it on the host (every byte of every live block loaded exactly once per
// step, no source at or above an entry's upto, the LDS image coop4_read's).
//
// A wave owns 64 work-list entries, one per lane ("slots" 0..63).  A block
// step loads one 64-byte block of every slot with four load instructions of
// 64 lanes x 16 bytes: instruction i serves slots 16i .. 16i+15, four lanes
// per slot.  The loads write LDS directly (LDS-DMA), lane l of instruction i
// at byte 1024 i + 16 l of the step's 4 KiB buffer, so the swizzle of
// coop4_store's image (piece q of slot c at 64 c + 16 ((q + c/4) & 3)) goes
// on the source address: lane l loads piece ((l & 3) - (l >> 4)) & 3.
//
// The kernel calls slot, piece, clamped_block, lds_instr_base and offer (it
// adds offer().first to the buffer's or the dummy line's address once, then
// 64 x clamped_block per step: source_offset's sum); buffer_of, lds_byte and
// read_byte state what the kernel's rotating buffer index, the hardware's
// lane-linear LDS write and coop4_read (sha1_lane.hpp) do, for the check.
#pragma once

#include <stdint.h>

namespace pvmap {

constexpr uint32_t kSlots = 64;        // entries (and lanes) per wave
constexpr uint32_t kInstr = 4;         // load instructions per block step
constexpr uint32_t kPieceBytes = 16;   // bytes per lane per load
constexpr uint32_t kBlockBytes = 64;
constexpr uint32_t kBufBytes = kSlots * kBlockBytes;  // one block step: 4 KiB
constexpr uint32_t kBufs = 5;          // block steps in LDS: the one compressed, four ahead
constexpr uint32_t kAhead = kBufs - 1;

// The slot lane `lane` loads for with instruction i.
constexpr uint32_t slot(uint32_t lane, uint32_t i) { return 16u * i + (lane >> 2); }
// The 16-byte piece of that slot's block it loads.
constexpr uint32_t piece(uint32_t lane) { return ((lane & 3u) - (lane >> 4)) & 3u; }
// The block of a slot with nb > 0 bulk blocks that step k loads: past the
// slot's last block, that block again (never a byte above it).
constexpr uint32_t clamped_block(uint32_t k, uint32_t nb) { return k < nb ? k : nb - 1u; }
// The LDS buffer of block step k.
constexpr uint32_t buffer_of(uint32_t k) { return k % kBufs; }
// Where the load lands in the buffer: instruction i's wave-uniform base,
// then 16 x lane (the hardware's rule, not the kernel's choice).
constexpr uint32_t lds_instr_base(uint32_t i) { return kSlots * kPieceBytes * i; }
constexpr uint32_t lds_byte(uint32_t lane, uint32_t i) { return lds_instr_base(i) + kPieceBytes * lane; }
// Where coop4_read (sha1_lane.hpp) expects piece q of slot c.
constexpr uint32_t read_byte(uint32_t c, uint32_t q) { return c * kBlockBytes + ((q + (c >> 2)) & 3u) * kPieceBytes; }

// What a slot offers its four loaders: where its first block lies -- a byte
// offset into its session buffer, or the 64-byte dummy line when the slot has
// nothing to load (no entry, a dropped entry, no whole block) -- and the
// block count the loaders clamp to (1 for the dummy line).  The kernel's
// owner lane computes exactly this and hands it round by shuffle.
struct Offer {
    bool dummy;
    uint32_t first;  // offset of block 0
    uint32_t nb;     // >= 1
};
constexpr Offer offer(bool live, uint32_t from, uint32_t nb) {
    return (live && nb) ? Offer{false, from, nb} : Offer{true, 0u, 1u};
}
// The byte offset (from the session buffer's or the dummy line's start) of
// lane `lane`'s load of step k from a slot with offer o.
constexpr uint32_t source_offset(const Offer& o, uint32_t k, uint32_t lane) {
    return o.first + kBlockBytes * clamped_block(k, o.nb) + kPieceBytes * piece(lane);
}

}  // namespace pvmap
