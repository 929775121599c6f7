/*
 * sha1chunk.h -- the batch entry points of the MI355X SHA-1 chunk engine
 * (libsha1chunk.so).  Plain C ABI: pointers, sizes, a `void *` HIP stream.
 *
 * These are the one new interface SURVEY.md 7.1 step 2 asks for.  The
 * reference has no batch API: every digest in /root/reference is produced by
 * a serial shahash() call (chunk.c:23 from make_chunks, chunk.c:180 from
 * get_chunk_hash <- job.c:218 verify_hash and chunk.c:208 verify_chunk_hash).
 * sha1chunk_hash_batch() replaces a loop of those calls; the reference-
 * signature functions in chunk_hash.h / sha.h are implemented on top of it.
 *
 * The library is two files: libsha1chunk.so (what callers link: these
 * symbols, a thin C front end on libc alone) and libsha1chunk_hip.so (the
 * HIP runtime and gfx950 kernels), which the front end loads from its own
 * directory on the first call that needs the GPU -- so a process whose
 * calls all take the host small-call path below never starts HIP.
 *
 * Error convention: 0 on success, a negative SHA1CHUNK_E* code otherwise
 * (never exit()); sha1chunk_last_error() returns a thread-local message.
 * There is no CPU fallback: without a usable gfx950 device every call
 * fails with SHA1CHUNK_ENODEV, the host-routed calls below included.
 *
 * Routing.  One message is one serial chain of
 * compressions: a GPU lane runs it at ~85 MB/s, a CPU core with the x86 SHA
 * extensions at ~2.5 GB/s.  So by default the reference's single-message
 * calls hash on the host: sha1chunk_compress_blocks / sha1chunk_finish (the
 * SHA1Update / SHA1Final trio), shahash and what is built on it
 * (get_chunk_hash, verify_hash, verify_chunk_hash's per-call path), and
 * sha1chunk_hash_fd (make_chunks) on a regular file of at most 4 MiB --
 * one 512 KiB chunk in ~0.2 ms instead of one lane's ~6 ms.  Every batch,
 * device and verify-queue entry point, and make_chunks on larger files and
 * streams, runs on the gfx950 kernels.  SHA1CHUNK_HOST_SMALL in the
 * environment (read once per process) changes this: "0" puts every call on
 * the kernels; "<bytes>" hashes every host call of at most that many bytes
 * on the host (batches, the trio, a regular file, a verify queue of batch 1
 * whose max length fits) and larger ones on the kernels.
 */
#ifndef SHA1CHUNK_H
#define SHA1CHUNK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHA1CHUNK_DIGEST_LEN 20
#define SHA1CHUNK_CHUNK_LEN 524288 /* constants.h:14 CHUNK_LEN */

enum {
    SHA1CHUNK_OK = 0,
    SHA1CHUNK_EINVAL = -1, /* bad argument                                   */
    SHA1CHUNK_ENODEV = -2, /* no HIP device / runtime                        */
    SHA1CHUNK_ENOMEM = -3, /* device or pinned allocation failed             */
    SHA1CHUNK_EHIP = -4,   /* HIP runtime error (see sha1chunk_last_error)   */
    SHA1CHUNK_EALIGN = -5, /* digest (4 B) / synthetic (8 B) buffer misaligned */
    SHA1CHUNK_EIO = -6     /* read error on a file descriptor                */
};

/* Where the buffers of sha1chunk_hash_batch / sha1chunk_verify_batch live. */
#define SHA1CHUNK_HOST 0u        /* host memory: staged through pinned buffers  */
#define SHA1CHUNK_DEVICE 1u      /* device memory of the current device         */
#define SHA1CHUNK_ALL_DEVICES 2u /* HOST only: shard the chunk list over every
                                    visible device, one host thread per device */

/* Kernel choice for the device entry points (AUTO picks by batch shape:
 * the split kernel up to two groups of 64 chunks per CU, the fused kernel
 * beyond; a ragged batch is hashed longest-first, and with more groups than
 * CUs through the mixed kernel, whose device-side plan splits the groups
 * between the one-group split shape and the fused kernel). */
enum {
    SHA1CHUNK_KERNEL_AUTO = 0,
    SHA1CHUNK_KERNEL_LANE = 1,  /* one lane per chunk, per-lane loads; any alignment   */
    SHA1CHUNK_KERNEL_FUSED = 2, /* one lane per chunk, schedule + rounds in registers,
                                   two 128-byte stages of per-lane loads ahead       */
    SHA1CHUNK_KERNEL_SPLIT = 3  /* schedule-producer + round-consumer wave pairs        */
};

/* digests[i*20 .. i*20+19] = SHA-1(base[offsets[i] .. offsets[i]+lengths[i])).
 * Synchronous.  Host mode accepts any alignment and overlapping chunks. */
int sha1chunk_hash_batch(const void *base, const uint64_t *offsets, const uint32_t *lengths,
                         size_t n, uint8_t *digests, unsigned flags);

/* One message's digest, routed as the reference's single-message calls are
 * (shahash, chunk.c:35-51, is this call): on the host by default, on the
 * kernels under SHA1CHUNK_HOST_SMALL=0 or above an explicit threshold
 * (routing above).  len <= 2^32 - 1 on the kernels. */
int sha1chunk_digest(const void *msg, uint64_t len, uint8_t digest[20]);

/* mismatch[i] = 0 if the digest of chunk i equals expected[i*20..], else 1
 * (the verify_hash() convention of job.c:217-228). */
int sha1chunk_verify_batch(const void *base, const uint64_t *offsets, const uint32_t *lengths,
                           size_t n, const uint8_t *expected, uint8_t *mismatch, unsigned flags);

/* Device-resident, asynchronous on `stream` (a hipStream_t, NULL = default).
 * All pointers are device pointers.  Returns after enqueueing.  Chunks may
 * start at any byte and lie anywhere in the buffer.  With KERNEL_AUTO (the
 * split shapes and the mixed kernel, whose loads are shared across the
 * wave) placement costs nothing and 16-byte aligned starts are ~10 % faster
 * in the fused shapes.  A forced KERNEL_FUSED or KERNEL_LANE loads one chunk
 * per lane and is layout-sensitive: chunks scattered far apart thrash the
 * address-translation cache (~2.8x slower measured). */
int sha1chunk_hash_device_async(const void *d_base, const uint64_t *d_offsets,
                                const uint32_t *d_lengths, size_t n, uint8_t *d_digests,
                                void *stream, int kernel);

/* Same for n equal chunks of chunk_len bytes laid back to back at d_base
 * (the make_chunks layout): no offset/length arrays needed. */
int sha1chunk_hash_uniform_async(const void *d_base, uint32_t chunk_len, size_t n,
                                 uint8_t *d_digests, void *stream, int kernel);

/* Device compare of computed vs expected digests -> mismatch bytes
 * (n at most 2^32 - 256 per call). */
int sha1chunk_compare_device_async(const uint8_t *d_digests, const uint8_t *d_expected,
                                   size_t n, uint8_t *d_mismatch, void *stream);

/* Hash a byte stream in 512 KiB chunks (the last one at its true length,
 * as make_chunks does, chunk.c:22-23) through a ring of pinned slots:
 * read -> H2D -> hash -> D2H, slots overlapping.  `reader` fills up to n bytes of dst
 * (pinned memory) and returns the count, 0 at end of stream, or (size_t)-1
 * on error; `sink` receives each completed run of digests in order.
 * Returns the number of chunks (>= 0) or a negative error. */
typedef size_t (*sha1chunk_reader_fn)(void *ctx, void *dst, size_t n);
typedef void (*sha1chunk_sink_fn)(void *ctx, size_t first_chunk, const uint8_t *digests,
                                  size_t count);
long sha1chunk_hash_stream(sha1chunk_reader_fn reader, void *reader_ctx, sha1chunk_sink_fn sink,
                           void *sink_ctx);
/* Same, when the caller knows how many bytes the reader will deliver
 * (size_hint > 0): slots are sized to the input (a small file does not
 * allocate 512 MiB pinned slots; a mid-size one is spread over all slots). */
long sha1chunk_hash_stream_sized(sha1chunk_reader_fn reader, void *reader_ctx,
                                 sha1chunk_sink_fn sink, void *sink_ctx, uint64_t size_hint);
/* File-descriptor convenience: up to max_chunks digests into `digests`;
 * *total_chunks (optional) gets the file's chunk count.  Hashes from the
 * fd's current offset and leaves it at the end of what was read.  A regular
 * file is read with parallel pread; with SHA1CHUNK_FILE_DEVICES=all (or a
 * count) in the environment it is split into contiguous chunk-aligned ranges
 * over that many devices, one pipeline each (make_chunks and the
 * make-chunks CLI go through here). */
long sha1chunk_hash_fd(int fd, uint8_t *digests, size_t max_chunks, size_t *total_chunks);

/* Streaming support for SHA1Update/SHA1Final: compress nblocks whole 64-byte
 * blocks (host memory) into the chaining value state[5]. */
int sha1chunk_compress_blocks(uint32_t state[5], const void *blocks, size_t nblocks);
/* Finish a stream: state[5] after prefix_bytes hashed bytes, then tail_len
 * (< 64) buffered bytes -> padded final block(s) -> 20-byte digest. */
int sha1chunk_finish(const uint32_t state[5], uint64_t prefix_bytes, const void *tail,
                     uint32_t tail_len, uint8_t digest[20]);

/* Synthetic corpus generated on the device: chunk c, 64-bit
 * LE word w = splitmix64(seed ^ (c << 24) ^ w), chunks first..first+count-1
 * written back to back, chunk_len bytes each (a multiple of 8 when count > 1,
 * else SHA1CHUNK_EALIGN).  One call fills at most 2^24 - 1 chunks (one
 * 256-thread workgroup per chunk, fewer than 2^32 work-items per launch): a
 * larger count is refused with SHA1CHUNK_EINVAL before anything is launched,
 * here and in the ragged variant; fill a larger corpus in several calls,
 * advancing `first` and the destination. */
int sha1chunk_synth_fill_async(void *d_dst, uint64_t first, uint64_t count, uint32_t chunk_len,
                               uint64_t seed, void *stream);
/* Ragged variant: chunk first+i of d_lengths[i] bytes at d_base + d_offsets[i]
 * (device arrays; every d_base + d_offsets[i] 8-byte aligned). */
int sha1chunk_synth_fill_ragged_async(void *d_base, const uint64_t *d_offsets,
                                      const uint32_t *d_lengths, uint64_t first, uint64_t count,
                                      uint64_t seed, void *stream);

/* ---- Asynchronous verify queue (the peer's receive path) --
 * The reference verifies each reassembled chunk synchronously inside its
 * select() loop (packet_handler.c:469-472 -> job.c:217 verify_hash).  A queue
 * verifies them asynchronously instead: submit() copies the chunk into pinned
 * memory (the caller may reuse its buffer at once) with its expected digest
 * and a tag, and poll() returns finished (tag, mismatch) pairs, mismatch
 * following verify_hash: 0 = match, 1 = mismatch -> re-GET.
 *
 * Default: a persistent drain kernel.  The chunks go into a ring in pinned
 * host memory (SHA1CHUNK_VQ_RING_MIB, default 1024) and are published in
 * groups of up to min(batch, 64); while fewer groups are in flight than the
 * drain has workgroups, each chunk goes out at once.  The copy engine
 * stages each group into a mirror of the ring in device memory
 * (SHA1CHUNK_VQ_DMA=0: the drain reads the pinned ring over PCIe instead).
 * The drain, one workgroup on each of SHA1CHUNK_VQ_CUS CUs (default 64;
 * all queues on a device share at most SHA1CHUNK_VQ_CU_BUDGET CUs, default
 * half, and queues beyond it launch per batch), hashes and compares the
 * groups and writes the results back to host memory; a workgroup exits
 * after SHA1CHUNK_VQ_IDLE_MS (default 20) without a claim or after
 * SHA1CHUNK_VQ_LIFE_MS (default 4) of work, and the next call starts it
 * again.  A lone chunk comes back after its own serial chain, with no
 * batch to fill and no flush.
 *
 * SHA1CHUNK_VQ_MODE=batch: batches are launched as kernels.  Once `batch`
 * submissions are pending (or on flush) the batch is hashed and
 * compared on the device asynchronously -- while two earlier batches are
 * still on the device a batch keeps growing by whole batches (up to 4 x
 * batch, at most 512; SHA1CHUNK_VQ_GROW=0 disables) and goes at the first
 * whole batch after one finishes (a submit or a poll notices); whole batches
 * therefore always come back through poll() without a flush.  Three batch
 * sets are in flight at once.
 *
 * batch == 1 with SHA1CHUNK_HOST_SMALL >= max_chunk_len (explicit opt-in): the
 * batch-size-1 host path.  Each submit hashes and compares its chunk on the
 * host before returning (0.2 ms per 512 KiB instead of a 6 ms device chain);
 * poll() returns the results in submission order.  A device is still
 * required.
 *
 * A queue's own streams (its drains' launch slots and its copy stream) are
 * created at a stream priority of their own (SHA1CHUNK_VQ_PRIO, default
 * "low"), so HIP maps them to other hardware queues than the caller's
 * default-priority streams: a persistent drain never sits in front of the
 * caller's own kernels.  Measured: a config-2 batch (4096 x 512 KiB)
 * launched on a fresh stream while four queues are continuously fed took
 * 6.25-6.47 ms against 6.02 solo (12-26 ms with the queues' streams at the
 * default priority); tests/test_gpu_vq_zero_copy.py::
 * test_wait_behind_busy_drains_is_bounded checks that the median stays
 * within 1.5x of solo.
 *
 * Every queue call takes the queue's lock, so several threads (receive
 * sessions) may share one queue; a call that waits (for ring space, or
 * poll(wait)) and submit()'s copy release the lock meanwhile, so the other
 * threads' calls go on.  destroy() must not overlap any other call on the
 * queue.  Persistent drains of all queues on one device hold at most
 * SHA1CHUNK_VQ_CU_BUDGET CUs (default half the device); a queue created
 * when that budget is spent uses batch launches.  The copy of submit() runs
 * on the calling thread, which has just filled the chunk and holds it in its
 * caches (SHA1CHUNK_VQ_THREADS=N > 1 splits it over N threads, the caller
 * and N - 1 helper threads per queue that spin briefly between submissions,
 * when no other submit is using them: measured slower, 1 / 4 receive threads
 * 7.7 / 26.8 GiB/s at N = 4 against 18.5 / 46.7 at the default 1);
 * reserve/commit has no copy.  Helper threads run on the CPUs of the GPU's
 * NUMA node (SHA1CHUNK_NUMA=off: anywhere); HIP's pinned allocation puts the
 * ring's pages on that node already (measured, every page).
 * Measured on 16384 x 512 KiB host chunks from 4 receive threads on the
 * GPU's node, one per L3 domain, pieces copied from a cache-resident
 * source: 45-48 GiB/s reserve/commit and submit alike, pass to pass, 0.88x
 * the PCIe copy rate; the same from a DRAM-resident source (DESIGN.md
 * section 6, profiles/vq_l3b.jsonl, bench_r06k*.log). */
typedef struct sha1chunk_vq sha1chunk_vq;
/* NULL on failure (sha1chunk_last_error() says why). */
sha1chunk_vq *sha1chunk_vq_create(size_t batch, uint32_t max_chunk_len);
int sha1chunk_vq_submit(sha1chunk_vq *q, const void *chunk, uint32_t len,
                        const uint8_t expected[20], uint64_t tag);
/* Zero-copy receive.  reserve() hands out a buffer of len (<= max_chunk_len)
 * bytes inside the queue's pinned ring -- the peer's per-session receive
 * buffer (reliable_udp.c:121 recv_session->data), filled in place as DATA
 * packets arrive (reliable_udp.c:339) -- and commit() verifies it where it
 * lies, with no copy (the call at packet_handler.c:472).  The buffer must
 * not change between commit() and its result; it stays valid after the
 * result is polled, until release() (after the caller copied the verified
 * chunk into its job buffer, reliable_udp.c:696-709, or dropped it).  A
 * reservation may also be released without a commit.  Unreleased buffers
 * hold ring space.  reserve() and submit() wait (bounded, SHA1CHUNK_VQ_WAIT_S,
 * default 120 s) for room while in-flight chunks or other threads'
 * reservations still filling hold it.  When the ring's oldest region is a
 * reserved buffer that is verified and not released, one of three things
 * happens:
 *  - it is the calling thread's own (its result polled or not; likewise its
 *    own reservation not yet committed): the call fails at once (NULL, resp.
 *    SHA1CHUNK_ENOMEM) -- room only that thread could free;
 *  - it is another thread's and its result is still unpolled: the call fails
 *    the same way after a 2 ms grace (room only a poll() and the release()
 *    after it free: when every receive thread waits in reserve() nobody
 *    polls).  Poll, release and retry;
 *  - it is another thread's and poll() has handed its result out: its owner
 *    is copying the chunk out and will release it, so the call waits for
 *    that release() like for an in-flight chunk.  If the bound runs out
 *    first the call fails with SHA1CHUNK_ENOMEM ("polled and not released"),
 *    not SHA1CHUNK_EHIP: the drain is fine.
 * In batch mode and on the batch-1 host path the buffer is ordinary host
 * memory (commit copies it, resp. hashes it in place). */
void *sha1chunk_vq_reserve(sha1chunk_vq *q, uint32_t len);
int sha1chunk_vq_commit(sha1chunk_vq *q, void *buf, uint32_t len, const uint8_t expected[20],
                        uint64_t tag);
int sha1chunk_vq_release(sha1chunk_vq *q, void *buf);
int sha1chunk_vq_flush(sha1chunk_vq *q);
/* Up to max finished results; wait != 0 blocks until everything submitted
 * before the call has finished (later submissions from other threads are not
 * waited for).  Returns the number written (>= 0) or a negative error. */
long sha1chunk_vq_poll(sha1chunk_vq *q, uint64_t *tags, uint8_t *mismatch, size_t max, int wait);
/* Submitted but not yet returned by poll(). */
size_t sha1chunk_vq_pending(const sha1chunk_vq *q);
void sha1chunk_vq_destroy(sha1chunk_vq *q);

/* ---- Progressive verify: hash a chunk while it is received ---------------
 * Every entry point above starts a chunk's hash when the chunk is complete,
 * so its verdict comes one serial chain (8192 compressions for 512 KiB,
 * ~6 ms on a GPU lane) after the last packet.  SHA-1 is serial inside a
 * message, so that chain cannot be shortened -- but it need not wait for the
 * last packet.  The reference's reliable UDP layer already knows which bytes
 * are final: cumulative_ack (reliable_udp.c:300-324) maintains
 * last_packet_acked, so bytes [0, 1484 x last_packet_acked) of
 * recv_session->data no longer change, while packets above that mark may
 * still land out of order (reliable_udp.c:331-350).  A progressive verifier
 * hashes the final bytes as the mark moves; after the last packet only the
 * last <= 1484 bytes (24 blocks) and the padding remain.
 *
 * create() makes `sessions` receive buffers of max_chunk_len bytes, each
 * starting on a 128-byte line, in pinned host memory that the device reads
 * directly (allocated like the persistent queue's PCIe-read ring), and one
 * private stream, on the device current at the call.  NULL on failure
 * (sha1chunk_last_error() says why); without a device there is no object:
 * no CPU fallback, and SHA1CHUNK_HOST_SMALL does not apply -- this object
 * always runs on the gfx950 kernel (csrc/sha1_progress.hip).
 *
 * open() starts a chunk of len bytes with its expected digest and a tag and
 * returns the session's buffer -- the peer's recv_session->data
 * (reliable_udp.c:121) -- or NULL when every session is in use or
 * len > max_chunk_len.
 *
 * advance(buf, ready) states that bytes [0, ready) are final: they will not
 * change again (rewriting them with the same contents, as a duplicate packet
 * does, is fine).  Bytes at and above ready may be written in any order and
 * overwritten freely; the device never reads them.  ready never decreases,
 * never exceeds len, and may move by any amount, 0 and 1 included.  The
 * session is complete when ready == len (for len == 0: advance(buf, 0)).
 * The call never waits for the device.
 *
 * hashed() reports how many bytes of the session the device has confirmed
 * hashed: a multiple of 64, or len once the verdict exists.
 *
 * poll() returns finished (tag, mismatch) pairs, mismatch as verify_hash
 * returns it (0 = match, 1 = mismatch -> re-GET), each tag exactly once, and
 * with digests != NULL each computed digest, 20 bytes per result (job.c:219-
 * 220 prints both hashes on a mismatch).  wait != 0 blocks until every
 * session completed before the call has its result.
 *
 * close() frees the session: before completion (the chunk is dropped, no
 * result is delivered) or after it (a verdict not yet polled still comes).
 * The buffer is not handed out again while an enqueued launch refers to it.
 * pending() counts completed sessions whose result poll() has not returned.
 *
 * Launch policy: advance() records the mark; advance(), hashed() and poll()
 * enqueue one kernel when fewer than two launches of the object are
 * outstanding (an event per launch slot, queried, never waited for) and
 * there is work -- a session with a new whole 64-byte block, or a completed
 * one.  While two launches are outstanding work accumulates and the next
 * launch takes all of it, so the launch rate is bounded by the kernel's time
 * with no threshold to tune.  No helper thread, no persistent kernel: every
 * kernel ends on its own and none waits on host memory.
 *
 * Errors: SHA1CHUNK_EINVAL for a buffer that is not an open session's, a
 * mark that moves back or beyond len, and an advance after completion.
 * Every call takes the object's lock, so several receive threads may share
 * one object; destroy() must not overlap any other call.
 *
 * Measured on MI355X (tools/pv_latency_bench, profiles/pv_latency.jsonl,
 * DESIGN.md section 6): a 512 KiB chunk fed in its 354 packets with the
 * hashing keeping up has its verdict 28.7-31.4 us (median of 24 chunks, six
 * runs; every chunk 27-35) after the final advance, against 6.05 ms for the
 * same chunk through sha1chunk_vq_submit.  That needs the chunk to arrive
 * slower than one lane hashes it (~50 MB/s from pinned memory; one launch
 * per packet up to 32 MB/s): fed all at once its verdict comes 10.2-10.8 ms
 * after the last byte, one lane's whole chain, more than the queue's.  64 /
 * 256 sessions fed at once hash at 167-476 / 141-174 MB/s in aggregate (each
 * lane's 16-byte reads over PCIe are the bound) on that kernel; the
 * shared-load kernel below is for them. */
typedef struct sha1chunk_pv sha1chunk_pv;
sha1chunk_pv *sha1chunk_pv_create(size_t sessions, uint32_t max_chunk_len);
void *sha1chunk_pv_open(sha1chunk_pv *p, uint32_t len, const uint8_t expected[20], uint64_t tag);
int sha1chunk_pv_advance(sha1chunk_pv *p, void *buf, uint32_t ready);
int sha1chunk_pv_hashed(sha1chunk_pv *p, const void *buf, uint32_t *bytes);
long sha1chunk_pv_poll(sha1chunk_pv *p, uint64_t *tags, uint8_t *mismatch, uint8_t *digests,
                       size_t max, int wait);
int sha1chunk_pv_close(sha1chunk_pv *p, void *buf);
size_t sha1chunk_pv_pending(const sha1chunk_pv *p);
void sha1chunk_pv_destroy(sha1chunk_pv *p);

/* Many sessions at once.  A receive loop that has just handled packets of k
 * sessions (one select() round of the peer) states all k marks in one call:
 * one lock and one launch decision instead of k, so the launch that follows
 * carries every session's new blocks instead of the first caller's alone.
 *
 * Apply n (buffer, mark) pairs in order, each exactly as sha1chunk_pv_advance
 * would, under one lock and with one launch decision at the end.  Stops at
 * the first pair advance() would refuse: returns its error, *applied (may be
 * NULL) = pairs applied before it, and the applied ones still go to the
 * device.  n == 0 is a pump.  Never waits for the device. */
int sha1chunk_burst_advance(sha1chunk_pv *p, void *const *bufs, const uint32_t *ready,
                            size_t n, size_t *applied);

/* Which kernel a launch takes: SHA1CHUNK_PV_KERNEL=auto|lane|shared, read by
 * create() (anything else: create fails, SHA1CHUNK_EINVAL).  `lane` is one
 * lane per session, each lane reading its own buffer (csrc/sha1_progress.hip);
 * `shared` lays a wave's loads out four lanes per session, so that one load
 * instruction reads 16 sessions' whole 64-byte blocks instead of 64 quarter
 * blocks (csrc/sha1_progress_shared.hip); both force the choice for every
 * launch.  `auto`, the default: a launch with a single work-list entry always
 * takes the lane kernel -- a lone session's path is the one measured above --
 * and a larger one the shared kernel from 64 entries that carry a whole block
 * (the smallest session count at which it measured faster, below).
 * The counters below say what an object's launches were.
 *
 * The rule counts the entries of one launch, not the object's sessions: an
 * object with fewer than 64 sessions, or a receive round in which fewer than
 * 64 sessions gained a whole block, stays on the lane kernel under `auto`;
 * set SHA1CHUNK_PV_KERNEL=shared to use the shared kernel there.
 *
 * Measured on MI355X (tools/pv_latency_bench run C, profiles/pv_shared.jsonl,
 * DESIGN.md section 6; median (min-max) of six runs in two sittings,
 * aggregate MB/s, lane / shared forced): fed one burst per round 4 sessions
 * 195 (181-210) / 208 (207-208), 16: 768 (732-878) / 829 (828-833), 64: 190
 * (143-239) / 2208 (1815-2333), 256: 176 (167-211) / 8633 (7384-9117); fed
 * one advance per packet 64: 217 (194-280) / 1531 (1150-1696), 256: 202
 * (158-463) / 2492 (2401-2562).  64 is the smallest measured count at which
 * the shared kernel's median passes the lane kernel's by more than the lane
 * kernel's spread.  Under `auto` (three runs): 64 sessions 1396 (1347-1615)
 * per packet / 1952 (1873-2324) per round, 256: 2274 (2203-2570) / 7460
 * (7385-8636); 4 and 16 sessions run on the lane kernel.  A lone session's
 * last-advance-to-verdict time is unchanged (29.2-31.0 us against the parent
 * build's 29.4-30.3, every chunk 27.9-32.5).  Not measured: session counts
 * between 16 and 64, several devices, a real congestion-controlled peer. */
typedef struct {
    uint64_t launches, launches_shared; /* kernels enqueued; of those, shared-load */
    uint64_t entries, blocks;           /* work-list entries and 64-byte blocks issued */
    uint32_t kernel;                    /* 0 auto, 1 lane, 2 shared */
    uint32_t depth;
} sha1chunk_progress_stats_t;
/* size = sizeof the caller's struct (fields beyond it are not written). */
int sha1chunk_progress_stats(sha1chunk_pv *p, sha1chunk_progress_stats_t *out, size_t size);

/* ---- Batched SHA1Init / SHA1Update / SHA1Final: many messages in pieces ---
 * The streaming trio of sha.h for N messages at once: each message has its
 * own context, its pieces lie anywhere in host or device memory, have any
 * length and arrive over any number of calls.  (sha1chunk_pv is the special
 * case of receive sessions in the library's own pinned buffers, fed as a
 * growing prefix, verify only; use it for that.)
 *
 * A context is the reference's SHA1Context (sha.h), passed as void * since
 * this header does not include sha.h: SHA1CHUNK_CONTEXT_BYTES (96) bytes,
 * totalLength (bits) at byte 0, hash[5] at byte 8, bufferLength at byte 28,
 * buffer at byte 32.  `contexts` is an array of n_contexts such structs,
 * 8-byte aligned.  Entry i (0 <= i < n) works on context index ? index[i] : i.
 *
 * Update.  After update, context c of entry i holds what SHA1Update(&ctx[c],
 *   base + offsets[i], lengths[i]) leaves: totalLength, hash, bufferLength
 *   and the first bufferLength bytes of buffer.  The buffer bytes at and
 *   above bufferLength are unspecified (stale bytes in the reference too).
 *   Nothing outside the 96 bytes is written.
 * Final.  After final, digests[20*i ..] holds what SHA1Final returns (digests
 *   may be NULL), and the context is left as SHA1Final leaves it: hash = the
 *   digest words, bufferLength = 0, totalLength = the padded bit count.
 * Init is SHA1Init.
 * Migration.  The bytes are the struct: a context moves between these calls
 *   and the library's SHA1Init / SHA1Update / SHA1Final by plain copy.
 * Duplicates.  A context may appear at most once per call.  The host forms
 *   check this: a duplicate, or an index[i] >= n_contexts, is refused with
 *   SHA1CHUNK_EINVAL and nothing is touched.  The device forms cannot see the
 *   list: an entry whose index is >= n_contexts is skipped by the kernels (no
 *   read or write through it, its digest left untouched), and so is an entry
 *   whose context has bufferLength > 63 (the reference would overrun its
 *   buffer; this library does not index with it).  Duplicates in a device
 *   call are UNDEFINED: the entries race on the context.
 * Ordering.  Calls that touch the same context must be ordered by the
 *   caller: the same stream, or the caller's own events.  The async forms
 *   never wait for the device.
 * Overlap.  Pieces must not overlap the contexts.
 * Argument checks (made before anything reaches the device): n == 0 is a
 *   successful no-op; null pointers with n > 0 and n above 2^32 - 1025 are
 *   SHA1CHUNK_EINVAL; a device digest buffer that is not 4-byte aligned is
 *   SHA1CHUNK_EALIGN; SHA1CHUNK_ALL_DEVICES is SHA1CHUNK_EINVAL.
 * Routing.  Batch entry points: always on the gfx950 kernels
 *   (csrc/sha1_update.hip and, for the whole blocks, the lane / fused / split
 *   kernels resumed from each context's chaining value; SHA1CHUNK_FORCE_KERNEL
 *   applies).  SHA1CHUNK_HOST_SMALL does not apply, as for sha1chunk_pv;
 *   without a device they return SHA1CHUNK_ENODEV.
 *
 * The host form of update stages contexts and pieces through one pinned
 * buffer of SHA1CHUNK_UPDATE_FILL_MIB (default 256) MiB of pieces per fill;
 * larger batches go in several fills, a larger piece is cut at multiples of
 * 64 bytes inside the library.  Copy and hashing do not overlap.
 *
 * Measured on MI355X (tools/update_batch_bench.py, profiles/update_batch.jsonl,
 * DESIGN.md section 6; device-resident, HIP events, median (min-max) of seven
 * repetitions in one run): 4096 contexts each fed a whole 512 KiB in one
 * update and then finalised take 6.083 (6.078-6.110) ms against 6.048
 * (6.043-6.109) for sha1chunk_hash_uniform_async on the same bytes; an update
 * with nothing to hash costs 0.056 ms and final 0.014 ms.  One update call of
 * 1484-byte pieces, calls enqueued back to back: 64 contexts 34.4 us per call
 * (2.76 GB/s in aggregate), 256: 57.7 us (6.58 GB/s), 4096: 64.7 us
 * (94.0 GB/s).  A lone context still hashes at one lane's rate.  Not
 * measured: the host forms, several devices. */
#define SHA1CHUNK_CONTEXT_BYTES 96

/* Device-resident, asynchronous on `stream`; all pointers are device pointers. */
int sha1chunk_init_device_async(void *d_contexts, size_t n_contexts, const uint32_t *d_index,
                                size_t n, void *stream);
int sha1chunk_update_device_async(void *d_contexts, size_t n_contexts, const uint32_t *d_index,
                                  const void *d_base, const uint64_t *d_offsets,
                                  const uint32_t *d_lengths, size_t n, void *stream);
/* d_digests: n x 20 bytes, 4-byte aligned, may be NULL. */
int sha1chunk_final_device_async(void *d_contexts, size_t n_contexts, const uint32_t *d_index,
                                 size_t n, uint8_t *d_digests, void *stream);

/* Synchronous; flags = SHA1CHUNK_HOST (everything in host memory) or
 * SHA1CHUNK_DEVICE (everything in device memory: the async form + a wait). */
int sha1chunk_update_batch(void *contexts, size_t n_contexts, const uint32_t *index,
                           const void *base, const uint64_t *offsets, const uint32_t *lengths,
                           size_t n, unsigned flags);
int sha1chunk_final_batch(void *contexts, size_t n_contexts, const uint32_t *index, size_t n,
                          uint8_t *digests, unsigned flags);

/* ---- Messages given as segment lists: reassembly on the device -------------
 * Every entry point above takes a message as one contiguous run of bytes.  A
 * chunk on the receive path is not one: 512 KiB arrive as 354 DATA packets
 * (353 x 1484 B + 436 B, each a 16-byte header and its payload in a datagram
 * of at most 1500 bytes) that land wherever the socket call put them, in
 * arrival order, and the reference copies every payload to
 * data + 1484 * (seq - 1) (reliable_udp.c:339-341).  These calls hash and
 * verify N messages from where their pieces lie -- a packet ring in pinned
 * memory needs no CPU payload copy -- and can hand back the reassembled bytes.
 *
 * Segment list (CSR), shared by all forms: segment s is seg_lengths[s] bytes
 *   at base + seg_offsets[s]; message i (0 <= i < n) is the concatenation, in
 *   order, of segments seg_first[i] .. seg_first[i+1]-1; seg_first has n + 1
 *   entries.  Segments may have any length (0 included) and any byte
 *   alignment, may overlap, and a segment's bytes may be listed again under
 *   another index for another message.  A message's length is the sum of its
 *   segments' lengths.
 * Reads.  The device reads a segment through the aligned 4-byte words that
 *   hold its bytes: the other bytes of the first and last such word may be
 *   read too, and nothing beyond (the rule of the update kernels).
 *
 * Device form (sha1chunk_gather_device_async): all pointers are device
 *   pointers; d_base may also be memory from sha1chunk_pinned_alloc.  Message
 *   i is written contiguously at d_dst + d_dst_offsets[i] and
 *   d_out_lengths[i] (the array may be NULL) receives its length.  Exactly the
 *   message's bytes are written: whole aligned 16-byte words inside it as
 *   vector stores, its first and last partial words byte by byte, so bytes
 *   around and between messages stay intact.  Asynchronous on `stream`; the
 *   call never waits for the device (the first call on a device allocates a
 *   128-byte counter); scratch comes from the stream-ordered allocator.
 * Skipped messages.  Message i is skipped -- no byte of d_dst written,
 *   d_out_lengths[i] = 0xFFFFFFFF -- when seg_first[i] > seg_first[i+1], when
 *   seg_first[i+1] > n_segments, when its length exceeds 2^32 - 2, or when
 *   d_dst_offsets[i] + length > dst_bytes, the way the update kernels skip a
 *   bad context index.  A message without bytes writes nothing and has length 0.
 * UNDEFINED in the device form (the device cannot see it): destination ranges
 *   of different messages that overlap; d_dst overlapping the sources or the
 *   arrays; and segment index ranges of two messages that overlap (possible
 *   only when seg_first decreases somewhere): their messages' bytes are
 *   unspecified.  Even then no load leaves the listed segments' words and no
 *   store leaves the destination ranges of the messages that are not skipped.
 *
 * Host-array forms (sha1chunk_hash_gather_batch, sha1chunk_verify_gather_batch):
 *   synchronous; the three segment arrays, digests, expected and mismatch are
 *   host arrays, and flags says where `base` lives: SHA1CHUNK_HOST (pageable
 *   or pinned host memory) or SHA1CHUNK_DEVICE.  digests[20*i ..] = SHA-1 of
 *   message i; mismatch[i] follows verify_hash (0 = match, 1 = mismatch).
 * Argument checks (made before anything reaches a device, outputs untouched):
 *   n == 0 is a successful no-op; null pointers with n > 0 (the segment arrays
 *   may be null when n_segments == 0), n or n_segments above 2^32 - 1025,
 *   SHA1CHUNK_ALL_DEVICES or unknown flags, a message whose segment range is
 *   reversed or reaches past n_segments, and a message longer than 2^32 - 2
 *   bytes are SHA1CHUNK_EINVAL (every condition the device form skips for;
 *   the destination is the library's own).
 * Routing.  Always on the gfx950 kernels; SHA1CHUNK_HOST_SMALL does not apply
 *   and there is no CPU fallback: without a device or the backend the calls
 *   return SHA1CHUNK_ENODEV.
 * Paths.  The batch goes in sub-batches of whole messages whose packed size
 *   (every message on a 128-byte line of a device stage) stays under
 *   SHA1CHUNK_GATHER_STAGE_MIB (1..65536, read per call, default 4096: 4096 x 512 KiB is one
 *   sub-batch; the default rests on no measurement); a sub-batch holds at
 *   least one message, however long.  With `base` in device memory, or in
 *   host memory the device reads in place (sha1chunk_pinned_alloc, or any
 *   other memory HIP reports as pinned), each sub-batch's segment arrays go
 *   up, the gather kernels (csrc/sha1_gather.hip) reassemble into the stage
 *   -- reading pinned memory over PCIe -- the stage is hashed as
 *   sha1chunk_hash_device_async hashes under SHA1CHUNK_KERNEL_AUTO
 *   (SHA1CHUNK_FORCE_KERNEL and SHA1CHUNK_SPLIT_UNIT apply) and compared on
 *   the device for verify, and only digests or flags come back.  With `base`
 *   in pageable memory (the compatibility path) the library's pack threads
 *   copy each sub-batch's segments contiguously into a pinned fill and
 *   sha1chunk_hash_batch's host path takes it from there; no gather kernel
 *   runs.  Sub-batches do not overlap: one is finished before the next is
 *   staged.  One host-form call runs at a time per device.
 *
 * Measured on MI355X (tools/gather_bench.py, profiles/gather.jsonl, DESIGN.md
 * section 6; 4096 x 512 KiB as 354 packets each in a permuted ring of
 * 1500-byte slots, median (min-max) of seven repetitions in one run).
 * Device-resident, HIP events: the gather alone 1.964 (1.957-1.991) ms, 1018
 * GiB/s of message bytes; gather then hash 7.978 (7.975-7.990) ms against
 * 6.019 (6.010-6.059) for sha1chunk_hash_uniform_async on the same bytes laid
 * contiguously: 1.96 ms (33 %) over it.  From sha1chunk_pinned_alloc memory
 * read in place: the gather 43.45 (43.43-43.51) ms, 46.0 GiB/s, beside 37.50
 * (37.47-37.52) ms, 53.3 GiB/s, for hipMemcpyAsync H2D of the same bytes;
 * sha1chunk_verify_gather_batch 51.03 (50.84-51.05) ms wall clock against
 * 44.05 (44.03-44.08) for sha1chunk_verify_batch from pinned contiguous
 * memory.  The pageable path: 88.9 (88.7-91.1) ms.  Not measured: several
 * sub-batches, ragged messages and other segment sizes, messages of more than
 * 2048 segments, several devices, these calls beside a busy verify queue. */

/* Pinned host memory the device can read in place (a packet ring): NULL and
 * sha1chunk_last_error() on failure, on bytes == 0 and without a device. */
void *sha1chunk_pinned_alloc(size_t bytes);
/* Frees it (NULL: a successful no-op).  No call may still be reading it. */
int sha1chunk_pinned_free(void *p);

int sha1chunk_gather_device_async(const void *d_base, const uint64_t *d_seg_offsets,
                                  const uint32_t *d_seg_lengths, size_t n_segments,
                                  const uint32_t *d_seg_first, size_t n, void *d_dst,
                                  const uint64_t *d_dst_offsets, uint64_t dst_bytes,
                                  uint32_t *d_out_lengths, void *stream);

int sha1chunk_hash_gather_batch(const void *base, const uint64_t *seg_offsets,
                                const uint32_t *seg_lengths, size_t n_segments,
                                const uint32_t *seg_first, size_t n, uint8_t *digests,
                                unsigned flags);
int sha1chunk_verify_gather_batch(const void *base, const uint64_t *seg_offsets,
                                  const uint32_t *seg_lengths, size_t n_segments,
                                  const uint32_t *seg_first, size_t n, const uint8_t *expected,
                                  uint8_t *mismatch, unsigned flags);

/* ---- Digest index: match chunk digests against a chunk list ---------------
 * Every path above ends in 20-byte digests, or in "does digest i equal
 * expected digest i".  The peer also asks which chunk a digest IS: it answers
 * a WHOHAS by looking each requested hash up in its has-chunks list and serves
 * a GET by find_chunk_idx_from_hash, a scan of the text file per call; and a
 * peer that holds a data file and the master list needs the has-chunks file
 * that names the file's chunks by their master ids (the reference's
 * tmp/B.haschunks: B.tar's two digests under ids 2 and 3 of C.masterchunks).
 * Both are one primitive: a set of m known digests, queried with n digests,
 * answering with positions.  It runs on the device because that is where the
 * digests are after the hash calls above: a lookup queued on the same stream
 * needs no synchronise between hash and match and returns 4 bytes per chunk.
 *
 * An index is built over a table of m digests -- digest p has position p -- and
 * grows by appends afterwards: the has-chunks set of a peer that is downloading
 * gains a digest with every chunk it accepts (the reference's
 * update_owned_chunks appends the hash to the has-chunks file, and
 * process_whohas_packet reads the file again on the next WHOHAS).  A lookup
 * answers, for every queried digest, the lowest admitted position that holds
 * it, or SHA1CHUNK_NO_MATCH.
 *
 * Appends.  Digest i of an append gets position size_before + i.  Where the
 *   call's skip array is not NULL and skip[i] != 0, the position is used up but
 *   the digest is NOT admitted: no lookup ever answers it.  With skip = the
 *   mismatch bytes of a compare, exactly the verified chunks join the set:
 *   hash -> compare -> append(skip = mismatch) on one stream is the receive
 *   path, with no trip to the host between the verdict and the set.
 *   sha1chunk_admit_batch is that sequence in one call.
 * Positions.  sha1chunk_index_size counts every position handed out, skipped
 *   ones included.  The host therefore knows the size when it enqueues, without
 *   asking the device, and several appends can be queued back to back.
 * Lookups after appends.  A lookup still answers the lowest admitted position
 *   of a digest.  Appending a digest that is already in the set uses up a
 *   position and changes no answer.  A skipped digest that is admitted nowhere
 *   else answers SHA1CHUNK_NO_MATCH; admitted later, it answers the later
 *   position.
 * Capacity.  An index has room for sha1chunk_index_capacity digests: m after
 *   create.  The slot array always has the slot count of the Layout paragraph
 *   for `capacity` digests, so it is never more than half full and every probe
 *   ends.  sha1chunk_index_reserve and the host sha1chunk_index_append grow the
 *   index (never shrink it); the host form at least doubles the capacity when
 *   it is full.  The device form never allocates: if size + k > capacity it
 *   returns SHA1CHUNK_EINVAL with an error text that names
 *   sha1chunk_index_reserve, writes nothing and leaves the index as it was.
 *   An index that is never appended to keeps its slot count and its answers.
 * Ordering.  An append is a write to the index.  The caller orders it against
 *   every lookup and every other append of that index as it would order a
 *   write to a buffer: on the same stream, or through events.  The host forms
 *   (append, lookup, admit_batch(SHA1CHUNK_HOST), match_*) take turns under the
 *   device's mutex on one stream of the library's and may run from several
 *   threads at once.  Two threads must not append through the device form at
 *   once.  reserve, and a host append that grows, wait for the whole device
 *   before they read and before they free the old arrays; like destroy, they
 *   must not overlap a device-form call on the same index.
 *
 * Table size.  m may be 0; every lookup then answers SHA1CHUNK_NO_MATCH.
 *   m <= 2^31 (SHA1CHUNK_EINVAL above).
 * Duplicates.  Duplicate digests in the table are legal and the lowest
 *   position wins: a sparse file has thousands of identical all-zero chunks,
 *   and the reference's find_chunk_idx_from_hash returns the first match too.
 * Device.  An index belongs to the device that was current at create.  A call
 *   made with another device current is SHA1CHUNK_EINVAL.
 *   SHA1CHUNK_ALL_DEVICES is SHA1CHUNK_EINVAL in create and in match_batch.
 * Completion.  create copies the table into memory the index owns, builds on a
 *   stream of the library's own and waits for it; afterwards any stream and
 *   any thread may look up.  A SHA1CHUNK_DEVICE table must be complete before
 *   the call.  Lookups from several threads at once are allowed (host-array
 *   calls on one device take turns).  destroy must not overlap another call.
 * Alignment and count.  Digest and id arrays are 4-byte aligned, as digest
 *   buffers are elsewhere (SHA1CHUNK_EALIGN).  n <= 2^32 - 256 per lookup, as
 *   for the compare kernel; n <= 2^32 - 1025 for match_batch, as for every
 *   batch that is hashed.
 * Refusals.  A refused call writes nothing to its outputs.  A NULL index,
 *   NULL arrays with n > 0, SHA1CHUNK_ALL_DEVICES or unknown flags and n too
 *   large are SHA1CHUNK_EINVAL; these and misalignment are refused before the
 *   backend is loaded.  n == 0 with a valid index is a successful no-op.
 *   Of the appends: a NULL index, NULL digests with k > 0, k above the lookup
 *   limit, a capacity or a total size above 2^31, SHA1CHUNK_ALL_DEVICES or
 *   unknown flags in admit_batch and an index that belongs to another device
 *   are SHA1CHUNK_EINVAL; digests that are not 4-byte aligned are
 *   SHA1CHUNK_EALIGN.  skip and mismatch are bytes and may sit at any
 *   alignment.  k == 0 is a successful no-op.
 * Routing.  The host forms go through the device: stage up, kernel, 4 n bytes
 *   back.  There is no host hash map and no routing knob
 *   (SHA1CHUNK_HOST_SMALL does not apply); a gfx950 device is required, as
 *   everywhere else, and without one the calls return SHA1CHUNK_ENODEV.
 * Paths of the match forms.  match_batch(SHA1CHUNK_HOST) and match_fd run the
 *   hash paths of sha1chunk_hash_batch and sha1chunk_hash_fd on the kernels,
 *   unchanged, and then look the digests up.  match_batch(SHA1CHUNK_DEVICE)
 *   does what sha1chunk_verify_batch(SHA1CHUNK_DEVICE) does with the lookup
 *   where the compare is: same stream, one synchronise; ids is a device array
 *   then.  match_fd hashes from the fd's offset and leaves it where
 *   sha1chunk_hash_fd would; it returns the number of ids written (at most
 *   max_chunks) and *total_chunks (optional) gets the file's chunk count.
 *   admit_batch(SHA1CHUNK_DEVICE) is sha1chunk_verify_batch(SHA1CHUNK_DEVICE)'s
 *   sequence with the append behind the compare: same stream, one synchronise,
 *   expected and mismatch device arrays; it refuses when capacity is short, as
 *   the device append does.  admit_batch(SHA1CHUNK_HOST) hashes as
 *   sha1chunk_hash_batch does, compares, and appends through the host form,
 *   which grows the index.
 *
 * Layout (csrc/sha1_index.hip, arithmetic in csrc/index_map.hpp).  An
 *   open-addressed array of position words in device memory: the smallest
 *   power of two >= 2 m slots, at least 8, so it is at most half full and
 *   every probe sequence ends at an empty slot.  A digest's home slot is a
 *   fixed integer mix of its first two words only; probing is linear; a slot
 *   carries no tag, so every occupied probe compares all five words against
 *   the table (a tag word per slot is a possible later optimisation).  The
 *   build kernel runs one lane per entry and touches slots with agent-scope
 *   atomics only; the lookup kernel is a later kernel with plain loads.  The
 *   append kernel is the build kernel with a base and a skip array; the rows
 *   of a call are copied into the table by an earlier operation on the stream,
 *   so no lane reads a row that its own launch wrote.  Growth copies the rows
 *   and runs one lane per old slot, which inserts what the slot holds into the
 *   new array: the old slots hold exactly the admitted digests.
 * Trust.  The table comes from local chunk files, which are trusted.  Digests
 *   that share their first 8 bytes share a home slot: a hostile list degrades
 *   the build and the lookups to linear chains and stays correct.
 *
 * Measured on MI355X (tools/index_bench.py, profiles/index.jsonl, DESIGN.md
 * section 6; random digests, every query a hit, median (min-max) of 20
 * repetitions in one run).  m = n = 16384 / 262144: create from device memory
 * 0.054 (0.053-0.058) / 0.244 (0.239-0.275) ms wall clock; the lookup kernel
 * alone 0.012 (0.012-0.017) / 0.072 (0.033-0.078) ms by HIP events; the host
 * form 0.059 / 0.399 ms wall clock.  The same answer by copying the digests to
 * the host and asking a Python dict: 0.96 / 74.3 ms, and 0.76 / 21.9 ms to
 * build the dict.  Behind sha1chunk_hash_uniform_async on 4096 x 512 KiB (5.790
 * ms, 5.777-5.814) the lookup adds 0.010 ms and the compare kernel -0.001 ms,
 * both inside that spread.  Not measured: tables with long chains or many
 * duplicates, misses, m above 262144, match_batch and match_fd, several
 * devices.
 *
 * Appends, measured on MI355X (tools/index_append_bench.py,
 * profiles/index_append.jsonl; random digests, every one
 * admitted, median (min-max) of 20 repetitions in one run, each on a fresh
 * index of m digests).  k = 1 / 64 / 4096 digests appended to m = 262144:
 * sha1chunk_index_append_device_async 0.008 (0.008-0.009) / 0.012
 * (0.012-0.017) / 0.015 (0.014-0.018) ms by HIP events; the host form with
 * room 0.026 / 0.030 / 0.038 ms wall clock; the host form that grows the index
 * 0.442 / 0.458 / 0.465 ms; sha1chunk_index_destroy plus
 * sha1chunk_index_create over the m + k digests from device memory, the only
 * way before appends existed, 0.474 / 0.492 / 0.491 ms in the same run.  To
 * m = 16384: 0.013 / 0.014 / 0.019 ms, 0.018 / 0.021 / 0.033 ms, 0.044 /
 * 0.048 / 0.060 ms growing, against 0.040 / 0.039 / 0.040 ms for destroy plus
 * create: at that size a growth costs as much as building anew, and more for
 * k = 4096.  Every figure is tens of microseconds, a few launches' worth; the
 * benefit is that the set follows the verdicts on the stream, not the time.
 * Not measured: skip masks, duplicates, chains, appends behind a hash,
 * admit_batch, create from host memory, several devices. */
#define SHA1CHUNK_NO_MATCH 0xFFFFFFFFu
typedef struct sha1chunk_index sha1chunk_index;

/* m digests of 20 bytes; digest p has position p.  flags: SHA1CHUNK_HOST or
 * SHA1CHUNK_DEVICE (where `digests` lies).  Synchronous.  NULL on failure
 * (sha1chunk_last_error() says why). */
sha1chunk_index *sha1chunk_index_create(const uint8_t *digests, size_t m, unsigned flags);
void sha1chunk_index_destroy(sha1chunk_index *ix); /* NULL is fine */
/* Positions handed out: m plus every appended digest, skipped ones included; 0 for NULL. */
size_t sha1chunk_index_size(const sha1chunk_index *ix);

/* Room for at least `capacity` digests (never shrinks; capacity <= 2^31). Synchronous. */
int sha1chunk_index_reserve(sha1chunk_index *ix, size_t capacity);
size_t sha1chunk_index_capacity(const sha1chunk_index *ix); /* 0 for NULL */

/* Digest i of the call gets position size_before + i.  Where d_skip is not NULL and
 * d_skip[i] != 0, the position is used up but the digest is NOT admitted: no lookup
 * ever answers it.  Device arrays, asynchronous on `stream`; never waits for the
 * device and never allocates (SHA1CHUNK_EINVAL when size + k > capacity). */
int sha1chunk_index_append_device_async(sha1chunk_index *ix, const uint8_t *d_digests, size_t k,
                                        const uint8_t *d_skip, void *stream);
/* The same for host arrays; synchronous; grows the index when it is full. */
int sha1chunk_index_append(sha1chunk_index *ix, const uint8_t *digests, size_t k,
                           const uint8_t *skip);

/* ids[i] = lowest position p with table[p] == digests[i], else SHA1CHUNK_NO_MATCH.
 * Device arrays, asynchronous on `stream`; never waits for the device. */
int sha1chunk_index_lookup_device_async(const sha1chunk_index *ix, const uint8_t *d_digests,
                                        size_t n, uint32_t *d_ids, void *stream);
/* The same for host arrays; synchronous. */
int sha1chunk_index_lookup(const sha1chunk_index *ix, const uint8_t *digests, size_t n,
                           uint32_t *ids);

/* Hash, then look up: the arguments of sha1chunk_hash_batch, ids instead of digests. */
int sha1chunk_match_batch(const sha1chunk_index *ix, const void *base, const uint64_t *offsets,
                          const uint32_t *lengths, size_t n, uint32_t *ids, unsigned flags);
/* The arguments of sha1chunk_verify_batch: verify, then append every digest
 * (skip = mismatch), so that exactly the verified chunks join the set. */
int sha1chunk_admit_batch(sha1chunk_index *ix, const void *base, const uint64_t *offsets,
                          const uint32_t *lengths, size_t n, const uint8_t *expected,
                          uint8_t *mismatch, unsigned flags);
/* The arguments of sha1chunk_hash_fd, ids instead of digests. */
long sha1chunk_match_fd(const sha1chunk_index *ix, int fd, uint32_t *ids, size_t max_chunks,
                        size_t *total_chunks);

/* Device management. */
int sha1chunk_device_count(void);
int sha1chunk_set_device(int device);
int sha1chunk_get_device(void);
/* PCI address ("dddd:bb:dd.f") of logical device `device`'s physical GPU:
 * tells apart the devices SHA1CHUNK_ALL_DEVICES / SHA1CHUNK_FILE_DEVICES
 * shard over (several logical devices map to one GPU only under
 * SHA1CHUNK_VIRTUAL_DEVICES, a test knob). */
int sha1chunk_device_pci_bus_id(int device, char *buf, size_t len);
/* Where a receive thread feeding a verify queue on `device` should run:
 * writes into `mask` (a Linux cpu_set_t, len >= sizeof(cpu_set_t); the rest
 * of len is zeroed) the CPUs of one L3 domain (one CCD on the MI355X boxes'
 * EPYC hosts) of the device's NUMA node, within the process's affinity mask
 * (its main thread's, whichever thread calls, pinned or not);
 * receive thread `slot` gets domain slot mod their count, so threads 0..k-1
 * land on k different domains.  *domains (if not NULL) receives that count.
 * With SHA1CHUNK_NUMA=off, or the node unknown, the domains of every allowed
 * CPU.  Returns the number of CPUs in the mask, or a negative error.  Use:
 *   cpu_set_t cs;
 *   if (sha1chunk_receive_cpus(sha1chunk_get_device(), i, &cs, sizeof cs, NULL) > 0)
 *       pthread_setaffinity_np(thread_i, sizeof cs, &cs);
 * Measured (16384 x 512 KiB, 4 receive threads): one
 * per domain held submit at 27.7-29.6 GiB/s where threads floating over the
 * node gave 23.8-36.2 run to run (the copy then on helper threads; on the
 * receive thread since, both run 46-47). */
int sha1chunk_receive_cpus(int device, unsigned slot, void *mask, size_t len, unsigned *domains);
/* Last error text of this thread ("" if none). */
const char *sha1chunk_last_error(void);
/* "gfx950:<kernels>" build identity, for logs. */
const char *sha1chunk_version(void);

#ifdef __cplusplus
}
#endif

#endif
