// rt_file.hip -- the stream and fd pipeline of the HIP backend
// (sha1chunk_hash_stream / sha1chunk_hash_fd, the make-chunks CLI): a ring of
// pipeline slots, each read into pinned memory -- by several pread threads for
// a regular file -- copied H2D and hashed on its own stream, over one device
// or a file's byte ranges over several.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

#include "par_read.hpp"
#include "sha1_runtime_internal.h"

using namespace s1rt;

namespace {
// Stream (file) pipeline: a ring of slots, each read into pinned memory,
// copied H2D and hashed on its own stream.  A slot's kernel takes ~7 ms
// however few chunks it holds (one chunk's serial chain), so slots must be
// large (512 MiB: ~10 ms of PCIe) and several in flight: with 2 slots each
// read waited for the kernel 2 slots back.  3 slots keep the slot streams
// plus the copy stream within the process's 4 hardware queues (more streams
// share queues and serialise kernels).  Measured on an 8 GiB file in the
// page cache (profiles/file_vq_r01.json): 2 x 256 MiB 29.6 GiB/s, 3 x 512 MiB
// 47.9 GiB/s (PCIe H2D 53.6).
// SHA1CHUNK_STREAM_SLOTS (2..8) / SHA1CHUNK_STREAM_SLOT_MIB (16..1024) for A/B.
int stream_slots() {
    static const int n = [] {
        const char* e = getenv("SHA1CHUNK_STREAM_SLOTS");
        return e ? std::min(kMaxSlots, std::max(2, atoi(e))) : 3;
    }();
    return n;
}
size_t stream_slot_bytes() {
    static const size_t b = [] {
        const char* e = getenv("SHA1CHUNK_STREAM_SLOT_MIB");
        const size_t mib = e ? std::min<size_t>(1024, std::max<size_t>(16, atoi(e))) : 512;
        return mib << 20;  // a multiple of SHA1CHUNK_CHUNK_LEN
    }();
    return b;
}

// H2D piece of the stream pipeline (SHA1CHUNK_STREAM_PIECE_MIB, 0 = whole slot)
size_t stream_piece_bytes() {
    static const size_t b = [] {
        const char* e = getenv("SHA1CHUNK_STREAM_PIECE_MIB");
        return static_cast<size_t>(e ? std::max(0, atoi(e)) : 64) << 20;
    }();
    return b;
}

// size_hint: bytes the reader will deliver, when known (regular files); it
// sizes the slots (par_read.hpp slot_geometry).
long hash_stream_sized(sha1chunk_reader_fn reader, void* reader_ctx, sha1chunk_sink_fn sink,
                       void* sink_ctx, uint64_t size_hint) {
    if (!reader) return fail(SHA1CHUNK_EINVAL, "null reader");
    Device* D;
    int rc = get_device(&D);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(D->mu);
    if ((rc = discard_in_flight(*D))) return rc;
    const int nslots = stream_slots();
    const s1file::SlotGeometry geo = s1file::slot_geometry(size_hint, nslots, stream_slot_bytes());
    const size_t slot_bytes = geo.slot_bytes, per_slot = geo.per_slot, meta = geo.meta;
    bool one_fill = geo.one_fill;
    size_t next = 0;  // index of the next slot's first chunk
    size_t pend_first[kMaxSlots] = {}, pend_m[kMaxSlots] = {};
    auto finish = [&](int w) -> int {
        Slot& s = D->slot[w];
        if (!s.busy) return SHA1CHUNK_OK;
        s.busy = false;
        HIP_TRY(hipEventSynchronize(s.done));
        if (sink) sink(sink_ctx, pend_first[w], static_cast<const uint8_t*>(s.hdig.p), pend_m[w]);
        return SHA1CHUNK_OK;
    };
    int which = 0;
    bool eof = false;
    for (size_t fill = 0; !eof; ++fill) {
        // streams on first use; a reader that delivers more than size_hint
        // leaves the one-fill path at its second slot
        if (fill == 1) one_fill = false;
        if ((rc = ensure_slots(*D, which + 1)) || (!one_fill && (rc = ensure_copy(*D)))) return rc;
        Slot& s = D->slot[which];
        const hipStream_t cs = one_fill ? s.stream : D->copy;
        if ((rc = finish(which))) return rc;
        if ((rc = s.hpin.ensure(meta + slot_bytes)) || (rc = s.dmem.ensure(meta + slot_bytes)) ||
            (rc = s.hdig.ensure(per_slot * 20)) || (rc = s.ddig.ensure(per_slot * 20)))
            return rc;
        uint8_t* h = static_cast<uint8_t*>(s.hpin.p);
        uint8_t* d = static_cast<uint8_t*>(s.dmem.p);
        // Read straight into pinned memory: the fread loop of make_chunks
        // (chunk.c:22), a slot of up to 1024 chunks at a time, read in pieces
        // whose H2D copies start as soon as each piece is in, so the copy
        // engine is not idle while a whole slot is read (the first slot
        // above all); the kernel still waits for the whole slot.
        const size_t piece = stream_piece_bytes() ? stream_piece_bytes() : slot_bytes;
        size_t got = 0, sent = 0;
        while (got < slot_bytes) {
            const size_t r = reader(reader_ctx, h + meta + got, std::min(piece, slot_bytes - got));
            if (r == (size_t)-1) return fail(SHA1CHUNK_EIO, "stream read error");
            if (r == 0) {
                eof = true;
                break;
            }
            got += r;
            if (got - sent >= piece && got < slot_bytes) {
                HIP_TRY(hipMemcpyAsync(d + meta + sent, h + meta + sent, got - sent, hipMemcpyHostToDevice,
                                       cs));
                sent = got;
            }
        }
        if (got == 0) break;
        const size_t m = (got + SHA1CHUNK_CHUNK_LEN - 1) / SHA1CHUNK_CHUNK_LEN;
        uint64_t* hoff = reinterpret_cast<uint64_t*>(h);
        uint32_t* hlen = reinterpret_cast<uint32_t*>(h + m * 8);
        for (size_t j = 0; j < m; ++j) {
            hoff[j] = meta + j * SHA1CHUNK_CHUNK_LEN;
            hlen[j] = static_cast<uint32_t>(
                std::min<size_t>(SHA1CHUNK_CHUNK_LEN, got - j * SHA1CHUNK_CHUNK_LEN));
        }
        HIP_TRY(hipMemcpyAsync(d + meta + sent, h + meta + sent, got - sent, hipMemcpyHostToDevice, cs));
        HIP_TRY(hipMemcpyAsync(d, h, m * 12, hipMemcpyHostToDevice, cs));  // offsets + lengths
        if ((rc = copies_issued(s, cs))) return rc;
        BatchArgs A{};
        A.base = d;
        A.off = reinterpret_cast<const uint64_t*>(d);
        A.len = reinterpret_cast<const uint32_t*>(d + m * 8);
        A.n = static_cast<uint32_t>(m);
        A.dig = static_cast<uint8_t*>(s.ddig.p);
        if ((rc = launch_checked(choose_kernel(SHA1CHUNK_KERNEL_AUTO, m, D->cus), A, s.stream, D->cus)))
            return rc;
        HIP_TRY(hipMemcpyAsync(s.hdig.p, s.ddig.p, m * 20, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipEventRecord(s.done, s.stream));
        s.busy = true;
        pend_first[which] = next;
        pend_m[which] = m;
        next += m;
        which = (which + 1) % nslots;
    }
    // remaining slots complete in issue order: the sink sees ascending indices
    for (int k = 0; k < nslots; ++k)
        if ((rc = finish((which + k) % nslots))) return rc;
    return static_cast<long>(next);
}

struct FdSink {
    uint8_t* out;
    size_t max;
};
static size_t fd_reader(void* ctx, void* dst, size_t n) {
    const int fd = *static_cast<int*>(ctx);
    for (;;) {
        const ssize_t r = read(fd, dst, n);
        if (r >= 0) return static_cast<size_t>(r);
        if (errno != EINTR) return (size_t)-1;
    }
}
// Regular files: ParFile and par_reader (par_read.hpp), whose counters are
// added up over the process for s1be_file_read_stats.
using s1file::ParFile;
static_assert(s1file::kMetaAlign == kAlign, "par_read.hpp lays the slot's metadata out on the device's lines");
constexpr sha1chunk_reader_fn par_reader = s1file::par_reader<>;
std::atomic<uint64_t> g_read_calls{0}, g_read_split{0}, g_read_max_parts{0}, g_read_short{0};
static void count_reads(const ParFile& f) {
    g_read_calls += f.calls;
    g_read_split += f.split_calls;
    g_read_short += f.short_parts;
    uint64_t seen = g_read_max_parts.load();
    while (seen < f.max_parts && !g_read_max_parts.compare_exchange_weak(seen, f.max_parts)) {
    }
}
static void fd_sink(void* ctx, size_t first, const uint8_t* dig, size_t count) {
    FdSink* s = static_cast<FdSink*>(ctx);
    for (size_t j = 0; j < count; ++j)
        if (first + j < s->max && s->out) memcpy(s->out + 20 * (first + j), dig + 20 * j, 20);
}

// SHA1CHUNK_FILE_DEVICES (make_chunks on a regular file): how many devices
// share the file -- "all", or a count (default 1).  Each device hashes a
// contiguous, chunk-aligned byte range with its own pread pool, host thread
// and pipeline; digests land in disjoint slices of the caller's array (the
// chunk list split per device, SURVEY.md 8e: no collective).
int file_devices(uint64_t bytes) {
    const char* e = getenv("SHA1CHUNK_FILE_DEVICES");
    if (!e) return 1;
    const int nd = device_count();
    if (nd <= 1) return 1;
    const int want = strcmp(e, "all") == 0 ? nd : std::max(1, std::min(nd, atoi(e)));
    // at least one chunk per device
    const uint64_t chunks = (bytes + SHA1CHUNK_CHUNK_LEN - 1) / SHA1CHUNK_CHUNK_LEN;
    return static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>(want, chunks)));
}

long hash_file_devices(int fd, off_t pos, off_t end, int nd, int read_threads, FdSink* sk) {
    const uint64_t L = SHA1CHUNK_CHUNK_LEN;
    const uint64_t chunks = (static_cast<uint64_t>(end - pos) + L - 1) / L;
    std::vector<s1file::DevRange> rg(nd);
    std::vector<std::string> errs(nd);
    std::vector<std::thread> th;
    const int caller_dev = t_dev;
    for (int g = 0; g < nd; ++g) {
        th.emplace_back([&, g] {
            t_dev = (caller_dev + g) % device_count();
            const uint64_t c0 = chunks * g / nd, c1 = chunks * (g + 1) / nd;
            const off_t a = pos + static_cast<off_t>(c0 * L);
            const off_t b = std::min(end, pos + static_cast<off_t>(c1 * L));
            PartPool pool(std::max(1, read_threads) - 1, near_cpus(g_dev[t_dev].id));
            ParFile f{fd, a, b, &pool};
            struct Shift {
                FdSink* sk;
                uint64_t c0;
            } sh{sk, c0};
            auto sink = [](void* ctx, size_t first, const uint8_t* dig, size_t count) {
                Shift* z = static_cast<Shift*>(ctx);
                fd_sink(z->sk, z->c0 + first, dig, count);
            };
            const long got = hash_stream_sized(par_reader, &f, sink, &sh, static_cast<uint64_t>(b - a));
            rg[g] = s1file::DevRange{got, c0, c1, b, f.pos};
            count_reads(f);
            if (got < 0) errs[g] = s1be_last_error();
        });
    }
    for (auto& t : th) t.join();
    // a range that came up short (the file shrank) ends the file there
    const s1file::FileReduce red = s1file::reduce_ranges(rg.data(), nd);
    if (red.bad >= 0) return fail(static_cast<int>(red.n), "device %d: %s", red.bad, errs[red.bad].c_str());
    (void)lseek(fd, red.pos, SEEK_SET);
    return red.n;
}
}  // namespace

extern "C" {

long s1be_hash_stream_sized(sha1chunk_reader_fn reader, void* reader_ctx,
                                 sha1chunk_sink_fn sink, void* sink_ctx, uint64_t size_hint) {
    return hash_stream_sized(reader, reader_ctx, sink, sink_ctx, size_hint);
}

long s1be_hash_fd(int fd, uint8_t* digests, size_t max_chunks, size_t* total_chunks) {
    FdSink sk{digests, max_chunks};
    struct stat st;
    const off_t pos = lseek(fd, 0, SEEK_CUR);
    long n;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && pos >= 0) {
        const char* e = getenv("SHA1CHUNK_READ_THREADS");
        const int read_threads = e ? std::max(1, atoi(e)) : 8;
        const off_t end = std::max(pos, st.st_size);
        const int nd = file_devices(static_cast<uint64_t>(end - pos));
        if (nd > 1) {
            n = hash_file_devices(fd, pos, end, nd, read_threads, &sk);
        } else {
            PartPool pool(read_threads - 1, near_cpus(g_dev[t_dev].id));
            ParFile f{fd, pos, end, &pool};
            n = hash_stream_sized(par_reader, &f, fd_sink, &sk, static_cast<uint64_t>(f.end - f.pos));
            count_reads(f);
            (void)lseek(fd, f.pos, SEEK_SET);
        }
    } else {
        n = hash_stream_sized(fd_reader, &fd, fd_sink, &sk, 0);
    }
    if (n < 0) return n;
    if (total_chunks) *total_chunks = static_cast<size_t>(n);
    return static_cast<long>(std::min(static_cast<size_t>(n), max_chunks));
}

// Diagnostics (tests/test_gpu_file_geometry.py; no front-end symbol): what the
// process's par_reader calls did so far -- out[0] calls, out[1] calls split
// over more than one part, out[2] the largest part count, out[3] parts that
// came up short; reset != 0 then zeroes them.
void s1be_file_read_stats(uint64_t out[4], int reset) {
    std::atomic<uint64_t>* const c[4] = {&g_read_calls, &g_read_split, &g_read_max_parts, &g_read_short};
    for (int i = 0; i < 4; ++i) {
        if (out) out[i] = c[i]->load();
        if (reset) c[i]->store(0);
    }
}

}  // extern "C"
