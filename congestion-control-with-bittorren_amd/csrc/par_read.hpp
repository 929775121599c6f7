// par_read.hpp -- the host arithmetic of the file pipeline (rt_file.hip), as
// plain C++ (no HIP) so that tools/par_read_check.cc can check it on the CPU
// against a fake file, under AddressSanitizer and ThreadSanitizer too:
//   - par_reader: one read of a regular file split over the threads of a
//     PartPool, each part a pread loop; the read primitive is a parameter;
//   - slot_geometry: the size of a pipeline slot for a known input size;
//   - reduce_ranges: what a file hashed as byte ranges over several devices
//     returns and where it leaves the fd.
#pragma once

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <sys/types.h>
#include <unistd.h>
#include <vector>

#include "../../include/sha1chunk.h"
#include "part_pool.hpp"

namespace s1file {

// ---- the parallel reader ---------------------------------------------------
struct SysPread {
    ssize_t operator()(int fd, void* buf, size_t n, off_t off) const { return ::pread(fd, buf, n, off); }
};

// Regular files: each slot is filled by several threads with pread -- one
// thread copies from the page cache at only ~5-10 GB/s, well under the PCIe
// rate the pipeline can take.  [pos, end) is what is left to read; the caller
// leaves the fd offset at pos afterwards, as a read() loop would leave it.
template <class Pread = SysPread>
struct ParFileT {
    int fd;
    off_t pos, end;
    s1host::PartPool* pool;
    Pread rd{};
    // diagnostics (s1be_file_read_stats adds them up over the process)
    uint64_t calls = 0;        // par_reader calls
    uint64_t split_calls = 0;  // of these, split over more than one part
    uint64_t max_parts = 0;    // largest part count of a call
    uint64_t short_parts = 0;  // parts that read less than their length (the file shrank)
};
using ParFile = ParFileT<>;

constexpr size_t kMinPiece = size_t(8) << 20;  // a part is at least this long

// A sha1chunk_reader_fn over a ParFileT<Pread>: reads min(n, end - pos) bytes
// at pos into dst with T = max(1, min(pool width, want / MinPiece)) parts of
// ceil(want / T) bytes, and returns the bytes read contiguously from pos --
// less than that only when a part met the end of the file early (the file
// shrank: end becomes the new pos, and the next call returns 0) -- or
// (size_t)-1 when a pread failed.
template <class Pread = SysPread, size_t MinPiece = kMinPiece>
size_t par_reader(void* ctx, void* dst, size_t n) {
    ParFileT<Pread>* f = static_cast<ParFileT<Pread>*>(ctx);
    ++f->calls;
    if (f->pos >= f->end) return 0;
    const size_t want = std::min<size_t>(n, static_cast<size_t>(f->end - f->pos));
    const int T = static_cast<int>(std::max<size_t>(1, std::min<size_t>(f->pool->width(), want / MinPiece)));
    const size_t piece = (want + T - 1) / T;
    f->split_calls += T > 1;
    f->max_parts = std::max<uint64_t>(f->max_parts, static_cast<uint64_t>(T));
    std::vector<size_t> got(T, 0);
    std::atomic<bool> bad{false};
    auto work = [&](int t) {
        const size_t lo = std::min(want, piece * t), len = std::min(want, lo + piece) - lo;
        uint8_t* d = static_cast<uint8_t*>(dst) + lo;
        while (got[t] < len) {
            const ssize_t r = f->rd(f->fd, d + got[t], len - got[t], f->pos + static_cast<off_t>(lo + got[t]));
            if (r < 0) {
                if (errno == EINTR) continue;
                bad = true;
                return;
            }
            if (r == 0) return;  // the file shrank under us
            got[t] += static_cast<size_t>(r);
        }
    };
    f->pool->run(static_cast<size_t>(T), [&](size_t t) { work(static_cast<int>(t)); });
    if (bad) return (size_t)-1;
    // bytes read contiguously from pos (a short piece ends the file)
    size_t total = 0;
    bool cut = false;
    for (int t = 0; t < T; ++t) {
        const size_t lo = std::min(want, piece * t), len = std::min(want, lo + piece) - lo;
        if (!cut) total += got[t];
        if (got[t] < len) {
            ++f->short_parts;
            if (!cut) f->end = f->pos + static_cast<off_t>(total);
            cut = true;
        }
    }
    f->pos += static_cast<off_t>(total);
    return total;
}

// ---- slot geometry of the stream pipeline ----------------------------------
constexpr size_t kMetaAlign = 128;  // = s1rt::kAlign (checked in rt_file.hip)
inline size_t round_up_to(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct SlotGeometry {
    size_t slot_bytes;  // data bytes of one slot: a multiple of SHA1CHUNK_CHUNK_LEN
    bool one_fill;      // a known size that fits one slot: slot 0 alone, copies on its stream
    size_t per_slot;    // chunks per slot (1024 per 512 MiB)
    size_t meta;        // bytes of offsets + lengths in front of the data
};

// size_hint: bytes the reader will deliver, when known (regular files), else
// 0; small inputs then get a slot just big enough (the pinned allocation is a
// one-process cost the make-chunks CLI pays on every run), mid-size inputs
// are spread over all slots so reads and copies overlap.  env_slot_bytes:
// the configured slot size (SHA1CHUNK_STREAM_SLOT_MIB).
inline SlotGeometry slot_geometry(uint64_t size_hint, int nslots, size_t env_slot_bytes) {
    const size_t L = SHA1CHUNK_CHUNK_LEN;
    SlotGeometry g;
    g.slot_bytes = env_slot_bytes;
    g.one_fill = false;
    if (size_hint) {
        // a hint within a chunk of 2^64 must not wrap to a slot of no bytes
        const size_t hint = static_cast<size_t>(std::min<uint64_t>(size_hint, UINT64_MAX - L));
        const size_t whole = round_up_to(hint, L);
        const size_t spread = std::max(size_t(64) << 20, round_up_to(hint / static_cast<size_t>(nslots), L));
        g.slot_bytes = std::min({g.slot_bytes, whole, spread});
        g.one_fill = whole <= g.slot_bytes;
    }
    g.per_slot = g.slot_bytes / L;
    g.meta = round_up_to(g.per_slot * 12, kMetaAlign);
    return g;
}

// ---- a file's byte ranges over several devices ------------------------------
// Device g hashes chunks [c0, c1) of the file, the bytes [.., end): got is
// its chunk count (negative: an error code) and stop the offset its reader
// reached.
struct DevRange {
    long got;
    uint64_t c0, c1;
    off_t end, stop;
};
struct FileReduce {
    long n;     // chunks hashed, in file order, up to the first short range; an error's code
    off_t pos;  // where the fd belongs (unset on error)
    int bad;    // the first device whose range failed before any came up short, or -1
};

// The first range that came up short (the file shrank) ends the file there:
// later ranges do not count, and the fd is left where that range's reader
// stopped, as a read() loop would leave it.  A range is short when it has
// fewer chunks than its share, or when its reader stopped before the range's
// end (the file ended inside the range's last chunk).
inline FileReduce reduce_ranges(const DevRange* r, int nd) {
    FileReduce out{0, 0, -1};
    for (int g = 0; g < nd; ++g) {
        if (r[g].got < 0) {
            out.n = r[g].got;
            out.bad = g;
            return out;
        }
        out.n += r[g].got;
        out.pos = r[g].stop;
        if (static_cast<uint64_t>(r[g].got) < r[g].c1 - r[g].c0 || r[g].stop < r[g].end) return out;
    }
    return out;
}

}  // namespace s1file
