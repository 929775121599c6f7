/*
 * reassembly_driver.c -- TEST INFRASTRUCTURE ONLY (oracle/Makefile `dropin`).
 *
 * Reassembles chunks with the reference peer's own receive-side code,
 * compiled unmodified and linked without chunk.o and sha.o against
 * libsha1chunk.so, and verifies them through the library's verify queue and
 * progressive verifier -- the patch of INTEGRATION.md section 3, run.  The
 * reference functions called here:
 *
 *   reliable_udp.c:108-131  build_udp_recv_session (its Malloc'ed data is
 *                           replaced by the library's buffer where the mode
 *                           says so)
 *   reliable_udp.c:300-324  cumulative_ack         (seqNo == last_packet_acked + 1)
 *   reliable_udp.c:331-350  copy_recv_packet_2_buf (every other in-window seqNo;
 *                           the choice ack_recv_data_packet makes at :425-431)
 *   reliable_udp.c:696-709  copy_chunk_2_job_buf   (on a match, before release)
 *   job.c:217-228           verify_hash            (mode plain)
 *   chunk.c                 read_chunk, hex2binary (the library's, by link)
 *
 * Nothing here hashes, and no socket is opened: ack_recv_data_packet and
 * process_data_packet send ACKs, so their two conditions are restated as the
 * driver's own (the stray-packet filter of packet_handler.c:460-464 in
 * deliver(), the completion test of :469 -- a datagram shorter than
 * UDP_MAX_PACK_SIZE -- right after it).
 *
 * usage: reassembly_driver <mode> <data file> <chunk-hash file> <scenario> <out dir>
 *   mode: plain | submit | reserve | pv | pv-burst
 *   (built with -DRSM_REFERENCE_ONLY, from the whole reference including its
 *    chunk.c and sha.c and without the library: plain only)
 *
 * scenario file, plain text:
 *   line 1:  <sessions S> <global seed> <subset %> <reorder %> <dup %> <stray %> <sync %>
 *            (sync: after that share of the advances the driver waits until
 *             the device has hashed up to the mark, like a peer whose next
 *             packet is late: what the device then reads next lies right
 *             above a mark whose following packet has not arrived)
 *   then one line per chunk:
 *            <seed> <short_last_early 0|1> <n> { <seqNo> <offset in body> <xor mask> <F|D> } x n
 *   F corrupts the first copy of that packet, D every later (duplicate) copy;
 *   corruptions and short_last_early apply to a chunk's first attempt only,
 *   the re-GET is delivered clean.
 *
 * The packet schedule of one (chunk, attempt) is a pure function of the
 * chunk's seed and the attempt (pick() below; tests/reassembly_replay.py is
 * the same function in Python).  How the S open sessions interleave comes
 * from the global seed and, in the asynchronous modes, from when results
 * arrive; no buffer's contents depend on it.
 *
 * Output: every line of the driver's own starts with "RSM " (the reference
 * functions print to stdout too).
 *   RSM RESULT <chunk> <attempt> <tag> <verdict> [<digest hex>]   (before release/close)
 *   RSM DROP <chunk> <attempt> <tag>            (pv modes: closed incomplete)
 *   RSM JOB <chunk>                             (job buffer written to <out>/job.bin)
 *   RSM STATS launches=.. launches_shared=.. entries=.. blocks=.. kernel=.. depth=..
 *   RSM COUNTS delivered=.. copied_dups=.. strays=.. stability_writes=.. ring_full=.. syncs=..
 *              (ring_full: reserve() found no room while a verified buffer was held)
 *   <out>/buf_<chunk>_<attempt>.bin   the session buffer when its result was
 *                                     polled (or when it was dropped)
 * Exit status 0, or 1 with "RSM ERROR ..." on any library error, a mark
 * violation, or a dropped tag that came back.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "chunk.h"
#include "constants.h"
#include "job.h"
#include "packet_handler.h"
#include "peer_utils.h"
#include "reliable_udp.h"
#include "utility.h"

#ifndef RSM_REFERENCE_ONLY
#include "sha1chunk.h"
#endif

#define BODY (UDP_MAX_PACK_SIZE - PACK_HEADER_BASE_LEN)         /* 1484 */
#define NPACK ((CHUNK_LEN + BODY - 1) / BODY)                   /* 354 */
#define LAST_BODY (CHUNK_LEN - (NPACK - 1) * BODY)              /* 436 */
#define MAX_ATTEMPT 3
#define MAX_CORR 16

enum { M_PLAIN, M_SUBMIT, M_RESERVE, M_PV, M_PVBURST };

typedef struct {
    int seq, off, mask, dup; /* dup: 0 = first copy, 1 = duplicate copies */
} corr_t;

typedef struct {
    uint64_t seed;
    int early, ncorr;
    corr_t corr[MAX_CORR];
} chunk_sc;

typedef struct {
    int state; /* 0 empty, 1 filling */
    int chunk, attempt;
    uint64_t tag, lcg;
    int force_dup;
    int moved; /* last_packet_acked moved in this round (pv-burst) */
    uint8_t count[NPACK + 2];
    udp_recv_session rs;
} sess_t;

typedef struct {
    int used, chunk, attempt;
    uint64_t tag;
    udp_recv_session rs;
} rec_t;

static int g_mode, g_S, g_K;
static int g_subset, g_reorder, g_dup, g_stray, g_sync;
static uint64_t g_lcg;
static chunk_sc *g_sc;
static uint8_t *g_data;
static vector g_hashes, g_peers;
static job_t g_job;
static vector g_todo;
static const char *g_out;
static sess_t *g_sess;
static rec_t *g_rec;
static int g_nrec;
static int *g_queue, g_qhead, g_qtail; /* chunk * 16 + attempt */
static uint64_t *g_dropped;
static int g_ndropped;
static unsigned long g_delivered, g_copied_dups, g_strays, g_stab, g_ring_full, g_syncs;
#ifndef RSM_REFERENCE_ONLY
static sha1chunk_vq *g_vq;
static sha1chunk_pv *g_pv;
#endif

static void die(const char *what) {
    fflush(stdout);
#ifndef RSM_REFERENCE_ONLY
    printf("RSM ERROR %s: %s\n", what, sha1chunk_last_error());
#else
    printf("RSM ERROR %s\n", what);
#endif
    fflush(stdout);
    exit(1);
}

/* An error of the driver's own (no library call failed). */
static void fatal(const char *what) {
    fflush(stdout);
    printf("RSM ERROR %s\n", what);
    fflush(stdout);
    exit(1);
}

static uint32_t lcg_next(uint64_t *x) {
    *x = *x * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(*x >> 33);
}

static int received(const udp_recv_session *rs, int seq) {
    return rs->recved_flags[seq - rs->last_packet_acked - 1] != 0;
}

/* The next sequence number a session is handed.  Window rule: a number in
 * [last_packet_acked + 1, min(last_acceptable_frame, 354)], duplicates
 * allowed.  The short last packet ends the session (packet_handler.c:469),
 * so it goes last -- or, with short_last_early, as soon as the window admits
 * it, packet 353 being held back until then. */
static int pick(sess_t *s) {
    const udp_recv_session *rs = &s->rs;
    const int lpa = rs->last_packet_acked, laf = rs->last_acceptable_frame;
    const chunk_sc *sc = &g_sc[s->chunk];
    const int first = s->attempt == 0;
    int lo = lpa + 1, hi;
    if (s->force_dup) {
        const int seq = s->force_dup;
        s->force_dup = 0;
        return seq;
    }
    if (first && sc->early) {
        if (laf >= NPACK) return NPACK;
        hi = laf < NPACK - 2 ? laf : NPACK - 2;
    } else {
        if (lo == NPACK) return NPACK;
        hi = laf < NPACK - 1 ? laf : NPACK - 1;
    }
    /* a packet whose duplicate is to be corrupted goes out of order as soon
     * as the window admits it, and its duplicate right behind it */
    if (first)
        for (int i = 0; i < sc->ncorr; ++i) {
            const corr_t *c = &sc->corr[i];
            if (c->dup && c->seq > lo && c->seq <= hi && !s->count[c->seq]) {
                s->force_dup = c->seq;
                return c->seq;
            }
        }
    if ((int)(lcg_next(&s->lcg) % 100) < g_stray) /* outside the window: filtered */
        return (lcg_next(&s->lcg) & 1) && lpa >= 1 ? lpa : laf + 1;
    if ((int)(lcg_next(&s->lcg) % 100) >= g_reorder) return lo;
    int seq = lo + (int)(lcg_next(&s->lcg) % (uint32_t)(hi - lo + 1));
    if (received(rs, seq) && (int)(lcg_next(&s->lcg) % 100) >= g_dup)
        while (received(rs, seq)) seq = seq == hi ? lo : seq + 1; /* lo is never received */
    return seq;
}

static int body_of(const sess_t *s, int seq, int copy, char *body) {
    const int blen = seq == NPACK ? LAST_BODY : BODY;
    memcpy(body, g_data + (size_t)s->chunk * CHUNK_LEN + (size_t)BODY * (seq - 1), blen);
    if (s->attempt == 0 && copy >= 0) {
        const chunk_sc *sc = &g_sc[s->chunk];
        for (int i = 0; i < sc->ncorr; ++i)
            if (sc->corr[i].seq == seq && sc->corr[i].dup == (copy > 0))
                body[sc->corr[i].off] ^= (char)sc->corr[i].mask;
    }
    return blen;
}

/* One DATA packet into the reference's session code.  Returns 0 stray,
 * 1 taken, 2 taken and the session is complete (short datagram). */
static int deliver(sess_t *s, int seq) {
    udp_recv_session *rs = &s->rs;
    char body[UDP_MAX_PACK_SIZE];
    packet_h hdr;
    handler_input in;
    if (seq <= rs->last_packet_acked || seq > rs->last_acceptable_frame) {
        ++g_strays;
        return 0;
    }
    const int was = received(rs, seq);
    const int blen = body_of(s, seq, s->count[seq], body);
    if (s->count[seq] < 255) ++s->count[seq];
    memset(&hdr, 0, sizeof hdr);
    memset(&in, 0, sizeof in);
    hdr.magicNo = 15441;
    hdr.versionNo = 1;
    hdr.packType = 3;
    hdr.headerLen = PACK_HEADER_BASE_LEN;
    hdr.packLen = (uint16_t)blen;
    hdr.seqNo = (uint32_t)seq;
    in.header = &hdr;
    in.body_buf = body;
    in.buf_len = PACK_HEADER_BASE_LEN + blen;
    in.recv_size = PACK_HEADER_BASE_LEN + blen;
    const int before = rs->last_packet_acked;
    if (before + 1 == seq)
        cumulative_ack(rs, &in, seq);
    else
        copy_recv_packet_2_buf(rs, &in);
    ++g_delivered;
    g_copied_dups += was;
    if (rs->last_packet_acked != before) s->moved = 1;
    return in.recv_size < UDP_MAX_PACK_SIZE ? 2 : 1;
}

static void dump(const udp_recv_session *rs, int chunk, int attempt) {
    char path[4096];
    snprintf(path, sizeof path, "%s/buf_%d_%d.bin", g_out, chunk, attempt);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(rs->data, 1, CHUNK_LEN, f) != CHUNK_LEN || fclose(f)) fatal("dump");
}

static void enqueue(int chunk, int attempt) {
    if (attempt > MAX_ATTEMPT) fatal("too many attempts (every re-GET of a chunk was rejected)");
    g_queue[g_qtail++] = chunk * 16 + attempt;
}

/* A verdict: what process_data_packet does at packet_handler.c:472-485. */
static void finish(rec_t *r, int verdict, const uint8_t *digest) {
    printf("RSM RESULT %d %d %llu %d", r->chunk, r->attempt, (unsigned long long)r->tag, verdict);
    if (digest) {
        printf(" ");
        for (int i = 0; i < 20; ++i) printf("%02x", digest[i]);
    }
    printf("\n");
    dump(&r->rs, r->chunk, r->attempt);
    if (verdict) enqueue(r->chunk, r->attempt + 1);
}

/* ... and on a match the copy into the job buffer, from the session buffer. */
static void copy_out(rec_t *r) {
    chunk_to_download *c = (chunk_to_download *)vec_get(&g_todo, r->chunk);
    if (c->chunk) fatal("a chunk verified twice");
    copy_chunk_2_job_buf(&r->rs, &g_job, r->chunk);
    printf("\n");
}

static rec_t *rec_new(const sess_t *s) {
    for (int i = 0; i < g_nrec; ++i)
        if (!g_rec[i].used) {
            g_rec[i].used = 1;
            g_rec[i].chunk = s->chunk;
            g_rec[i].attempt = s->attempt;
            g_rec[i].tag = s->tag;
            g_rec[i].rs = s->rs;
            return &g_rec[i];
        }
    fatal("record table full");
    return NULL;
}

#ifndef RSM_REFERENCE_ONLY
static void expected_of(int chunk, uint8_t want[20]) {
    hex2binary((char *)vec_get(&g_hashes, chunk), 40, want);
}

/* A verified buffer stays valid after its result is polled, until release():
 * one verified reservation at a time is kept unreleased while the sessions
 * go on reserving, until the ring has no room left without it (reserve()
 * fails: room only this thread can free) or kHoldReserves reservations have
 * been made, and only then copied into the job buffer and released. */
enum { kHoldReserves = 200 };
static rec_t *g_held;
static int g_held_reserves;

static void release_held(void) {
    if (!g_held) return;
    copy_out(g_held);
    if (sha1chunk_vq_release(g_vq, g_held->rs.data)) die("vq_release of the held buffer");
    g_held->used = 0;
    g_held = NULL;
}

/* Results that are ready (wait = 0) or everything in flight (wait = 1). */
static long harvest(int wait) {
    uint64_t tags[64];
    uint8_t bad[64], dig[64 * 20];
    long total = 0;
    for (;;) {
        long k;
        if (g_pv) {
            k = sha1chunk_pv_poll(g_pv, tags, bad, dig, 64, wait);
        } else {
            if (wait && sha1chunk_vq_flush(g_vq)) die("vq_flush");
            k = sha1chunk_vq_poll(g_vq, tags, bad, 64, wait);
        }
        if (k < 0) die("poll");
        for (long i = 0; i < k; ++i) {
            rec_t *r = NULL;
            for (int d = 0; d < g_ndropped; ++d)
                if (g_dropped[d] == tags[i]) fatal("a dropped session's tag came back from poll");
            for (int j = 0; j < g_nrec; ++j)
                if (g_rec[j].used && g_rec[j].tag == tags[i]) r = &g_rec[j];
            if (!r) fatal("poll returned an unknown tag");
            if (bad[i] > 1) fatal("poll returned a verdict that is neither 0 nor 1");
            finish(r, bad[i], g_pv ? dig + 20 * i : NULL);
            if (g_mode == M_RESERVE && !bad[i] && !g_held) {
                g_held = r; /* copied out and released later: release_held() */
                g_held_reserves = 0;
                continue;
            }
            if (!bad[i]) copy_out(r);
            if (g_pv) {
                if (sha1chunk_pv_close(g_pv, r->rs.data)) die("pv_close");
            } else if (g_mode == M_RESERVE) {
                if (sha1chunk_vq_release(g_vq, r->rs.data)) die("vq_release");
            } else {
                free(r->rs.data);
            }
            r->used = 0;
        }
        total += k;
        if (k < 64) break;
    }
    return total;
}

static int inflight(void) {
    int n = 0;
    for (int j = 0; j < g_nrec; ++j) n += g_rec[j].used;
    return n;
}

static void *library_buffer(int chunk, uint64_t tag) {
    uint8_t want[20];
    expected_of(chunk, want);
    for (int tries = 0;; ++tries) {
        void *p = g_pv ? sha1chunk_pv_open(g_pv, CHUNK_LEN, want, tag) : sha1chunk_vq_reserve(g_vq, CHUNK_LEN);
        if (p) {
            if (g_held && ++g_held_reserves >= kHoldReserves) release_held();
            return p;
        }
        /* no room: only results polled and buffers given back make some (a
         * session closed with a launch in flight comes free by itself) */
        if (tries > 20000) die(g_pv ? "pv_open" : "vq_reserve");
        if (g_held) {
            release_held();
            ++g_ring_full;
        } else if (inflight())
            harvest(1);
        else
            usleep(50);
    }
}

static void check_mark(const sess_t *s, uint32_t mark) {
    uint32_t h = 0;
    if (sha1chunk_pv_hashed(g_pv, s->rs.data, &h)) die("pv_hashed");
    if (h > mark || (h % 64 && h != CHUNK_LEN)) {
        printf("RSM ERROR mark violation: chunk %d attempt %d hashed %u mark %u\n", s->chunk, s->attempt, h, mark);
        fflush(stdout);
        exit(1);
    }
    if ((int)(lcg_next(&g_lcg) % 100) >= g_sync) return;
    for (int spins = 0; h < (mark & ~63u) && h != CHUNK_LEN; ++spins) {
        if (spins > 500000) fatal("the device did not reach the mark within 5 s");
        usleep(10);
        if (sha1chunk_pv_hashed(g_pv, s->rs.data, &h)) die("pv_hashed");
    }
    ++g_syncs;
}

/* Between a commit and its result the committed buffer must stay as it is
 * while the peer goes on serving its other sessions: rewrite an in-window
 * duplicate into every other open session's own buffer. */
static void stability_writes(const sess_t *committed) {
    for (int i = 0; i < g_S; ++i) {
        sess_t *o = &g_sess[i];
        if (o == committed || o->state != 1) continue;
        const udp_recv_session *rs = &o->rs;
        for (int seq = rs->last_packet_acked + 2; seq <= rs->last_acceptable_frame && seq <= NPACK; ++seq)
            if (received(rs, seq)) {
                char body[UDP_MAX_PACK_SIZE];
                packet_h hdr;
                handler_input in;
                memset(&hdr, 0, sizeof hdr);
                memset(&in, 0, sizeof in);
                hdr.packLen = (uint16_t)body_of(o, seq, -1, body);
                for (int b = 0; b < hdr.packLen; ++b) body[b] = (char)~body[b]; /* must not land */
                hdr.seqNo = (uint32_t)seq;
                in.header = &hdr;
                in.body_buf = body;
                in.recv_size = PACK_HEADER_BASE_LEN + hdr.packLen;
                copy_recv_packet_2_buf(&o->rs, &in);
                ++g_stab;
                break;
            }
    }
}
#endif

static uint32_t mark_of(const udp_recv_session *rs) {
    const uint64_t m = (uint64_t)BODY * (uint64_t)rs->last_packet_acked;
    return m < CHUNK_LEN ? (uint32_t)m : CHUNK_LEN;
}

static void open_session(sess_t *s, int item) {
    memset(s, 0, sizeof *s);
    s->chunk = item / 16;
    s->attempt = item % 16;
    s->tag = 0x1000u + (uint64_t)item;
    s->lcg = g_sc[s->chunk].seed ^ (0x9E3779B97F4A7C15ULL * (uint64_t)(s->attempt + 1));
    build_udp_recv_session(&s->rs, 1, (char *)vec_get(&g_hashes, s->chunk), &g_peers);
#ifndef RSM_REFERENCE_ONLY
    if (g_mode == M_RESERVE || g_mode == M_PV || g_mode == M_PVBURST) {
        free(s->rs.data);
        s->rs.data = (char *)library_buffer(s->chunk, s->tag);
    }
#endif
    memset(s->rs.data, 0xA5, CHUNK_LEN);
    s->state = 1;
}

/* The session received its short last datagram: packet_handler.c:469-495. */
static void complete(sess_t *s) {
    if (g_mode == M_PLAIN) {
        rec_t *r = rec_new(s);
        const int verdict = verify_hash(s->rs.chunk_hash, s->rs.data);
        finish(r, verdict, NULL);
        if (!verdict) copy_out(r);
        free(r->rs.data);
        r->used = 0;
    }
#ifndef RSM_REFERENCE_ONLY
    else if (g_mode == M_SUBMIT || g_mode == M_RESERVE) {
        uint8_t want[20];
        expected_of(s->chunk, want);
        rec_new(s);
        if (g_mode == M_SUBMIT) {
            if (sha1chunk_vq_submit(g_vq, s->rs.data, CHUNK_LEN, want, s->tag)) die("vq_submit");
        } else {
            if (sha1chunk_vq_commit(g_vq, s->rs.data, CHUNK_LEN, want, s->tag)) die("vq_commit");
            stability_writes(s);
        }
    } else if (s->rs.last_packet_acked == NPACK) {
        rec_new(s); /* the mark CHUNK_LEN has been stated: the verdict comes by poll */
    } else {
        /* holes below the short packet: the verifier cannot complete.  Drop
         * the session with launches possibly in flight and re-GET. */
        printf("RSM DROP %d %d %llu\n", s->chunk, s->attempt, (unsigned long long)s->tag);
        dump(&s->rs, s->chunk, s->attempt);
        g_dropped[g_ndropped++] = s->tag;
        if (sha1chunk_pv_close(g_pv, s->rs.data)) die("pv_close of a dropped session");
        enqueue(s->chunk, s->attempt + 1);
    }
#endif
    s->state = 0;
}

static void usage(void) {
    fprintf(stderr, "usage: reassembly_driver plain|submit|reserve|pv|pv-burst <data> <chunk hashes> <scenario> <out dir>\n");
    exit(2);
}

int main(int argc, char **argv) {
    static const char *modes[] = {"plain", "submit", "reserve", "pv", "pv-burst"};
    if (argc != 6) usage();
    g_mode = -1;
    for (int i = 0; i < 5; ++i)
        if (!strcmp(argv[1], modes[i])) g_mode = i;
    if (g_mode < 0) usage();
#ifdef RSM_REFERENCE_ONLY
    if (g_mode != M_PLAIN) usage();
#endif
    g_out = argv[5];

    init_vector(&g_hashes, CHUNK_HASH_SIZE);
    read_chunk(argv[3], &g_hashes);
    g_K = g_hashes.len;
    if (g_K <= 0) fatal("no chunk hashes");

    FILE *f = fopen(argv[4], "r");
    if (!f) fatal("scenario file");
    unsigned long long gseed;
    if (fscanf(f, "%d %llu %d %d %d %d %d", &g_S, &gseed, &g_subset, &g_reorder, &g_dup, &g_stray, &g_sync) != 7 ||
        g_S < 1 || g_subset < 1)
        fatal("scenario header");
    g_lcg = gseed;
    g_sc = (chunk_sc *)calloc(g_K, sizeof *g_sc);
    for (int c = 0; c < g_K; ++c) {
        unsigned long long seed;
        if (fscanf(f, "%llu %d %d", &seed, &g_sc[c].early, &g_sc[c].ncorr) != 3 || g_sc[c].ncorr > MAX_CORR)
            fatal("scenario line");
        g_sc[c].seed = seed;
        for (int i = 0; i < g_sc[c].ncorr; ++i) {
            corr_t *k = &g_sc[c].corr[i];
            char kind;
            if (fscanf(f, "%d %d %d %c", &k->seq, &k->off, &k->mask, &kind) != 4) fatal("scenario corruption");
            k->dup = kind == 'D';
            const int blen = k->seq == NPACK ? LAST_BODY : BODY;
            if (k->seq < 1 || k->seq > NPACK || k->off < 0 || k->off >= blen) fatal("corruption outside the chunk");
            /* packets 1 and 354 never arrive out of order, so have no in-window duplicate */
            if (k->dup && (k->seq == 1 || k->seq == NPACK || (g_sc[c].early && k->seq == NPACK - 1)))
                fatal("no duplicate of that packet can be delivered");
        }
    }
    fclose(f);

    g_data = (uint8_t *)malloc((size_t)g_K * CHUNK_LEN);
    f = fopen(argv[2], "rb");
    if (!f || !g_data || fread(g_data, CHUNK_LEN, g_K, f) != (size_t)g_K) fatal("data file");
    fclose(f);

    /* one peer, the sender of every session; the job's chunk list */
    peer_info_t peer;
    memset(&peer, 0, sizeof peer);
    peer.id = 1;
    strcpy(peer.ip, "127.0.0.1");
    peer.port = 1;
    init_vector(&g_peers, sizeof(peer_info_t));
    vec_add(&g_peers, &peer);
    memset(&g_job, 0, sizeof g_job);
    init_vector(&g_todo, sizeof(chunk_to_download));
    for (int c = 0; c < g_K; ++c) {
        chunk_to_download ch;
        memset(&ch, 0, sizeof ch);
        strcpy(ch.chunk_hash, (char *)vec_get(&g_hashes, c));
        ch.chunk_id = (size_t)c;
        vec_add(&g_todo, &ch);
    }
    g_job.chunks_to_download = &g_todo;

    g_sess = (sess_t *)calloc(g_S, sizeof *g_sess);
    g_nrec = g_K * (MAX_ATTEMPT + 1);
    g_rec = (rec_t *)calloc(g_nrec, sizeof *g_rec);
    g_queue = (int *)calloc((size_t)g_K * (MAX_ATTEMPT + 2), sizeof *g_queue);
    g_dropped = (uint64_t *)calloc(g_nrec, sizeof *g_dropped);
    for (int c = 0; c < g_K; ++c) enqueue(c, 0);

#ifndef RSM_REFERENCE_ONLY
    if (g_mode == M_SUBMIT || g_mode == M_RESERVE) {
        g_vq = sha1chunk_vq_create((size_t)g_S, CHUNK_LEN);
        if (!g_vq) die("vq_create");
    } else if (g_mode == M_PV || g_mode == M_PVBURST) {
        g_pv = sha1chunk_pv_create((size_t)g_S, CHUNK_LEN);
        if (!g_pv) die("pv_create");
    }
    void **bufs = (void **)calloc(g_S, sizeof *bufs);
    uint32_t *marks = (uint32_t *)calloc(g_S, sizeof *marks);
#endif

    for (;;) {
        int open = 0;
        for (int i = 0; i < g_S; ++i) {
            if (g_sess[i].state == 0 && g_qhead < g_qtail) open_session(&g_sess[i], g_queue[g_qhead++]);
            open += g_sess[i].state;
        }
        if (!open) {
#ifndef RSM_REFERENCE_ONLY
            if (g_held) {
                release_held();
                continue;
            }
            if (g_mode != M_PLAIN && inflight()) {
                harvest(1);
                continue;
            }
#endif
            if (g_qhead == g_qtail) break;
            continue;
        }
        /* one select() round: one packet to each of a seeded subset */
        for (int i = 0; i < g_S; ++i) {
            sess_t *s = &g_sess[i];
            if (s->state != 1 || (int)(lcg_next(&g_lcg) % 100) >= g_subset) continue;
            s->moved = 0;
            const int got = deliver(s, pick(s));
#ifndef RSM_REFERENCE_ONLY
            if (g_mode == M_PV && s->moved) {
                if (sha1chunk_pv_advance(g_pv, s->rs.data, mark_of(&s->rs))) die("pv_advance");
                check_mark(s, mark_of(&s->rs));
                s->moved = 0;
            }
#endif
            if (got == 2 && g_mode != M_PVBURST) complete(s);
            if (got == 2 && g_mode == M_PVBURST) s->state = 2; /* completes after the round's burst */
        }
#ifndef RSM_REFERENCE_ONLY
        if (g_mode == M_PVBURST) {
            size_t n = 0, applied = 0;
            for (int i = 0; i < g_S; ++i)
                if (g_sess[i].state && g_sess[i].moved) {
                    bufs[n] = g_sess[i].rs.data;
                    marks[n++] = mark_of(&g_sess[i].rs);
                }
            if (sha1chunk_burst_advance(g_pv, bufs, marks, n, &applied) || applied != n) die("burst_advance");
            for (int i = 0; i < g_S; ++i) {
                sess_t *s = &g_sess[i];
                if (s->state && s->moved) check_mark(s, mark_of(&s->rs));
                s->moved = 0;
                if (s->state == 2) complete(s);
            }
        }
        if (g_mode != M_PLAIN) harvest(0);
#endif
    }

    /* the job buffers of the chunks that verified (write_data_outputfile's loop) */
    char path[4096];
    snprintf(path, sizeof path, "%s/job.bin", g_out);
    f = fopen(path, "wb");
    if (!f) fatal("job.bin");
    for (int c = 0; c < g_K; ++c) {
        chunk_to_download *ch = (chunk_to_download *)vec_get(&g_todo, c);
        if (!ch->chunk) continue;
        if (fwrite(ch->chunk, 1, CHUNK_LEN, f) != CHUNK_LEN) fatal("job.bin");
        printf("RSM JOB %d\n", c);
    }
    fclose(f);
#ifndef RSM_REFERENCE_ONLY
    if (g_pv) {
        sha1chunk_progress_stats_t st;
        memset(&st, 0, sizeof st);
        if (sha1chunk_progress_stats(g_pv, &st, sizeof st)) die("progress_stats");
        printf("RSM STATS launches=%llu launches_shared=%llu entries=%llu blocks=%llu kernel=%u depth=%u\n",
               (unsigned long long)st.launches, (unsigned long long)st.launches_shared,
               (unsigned long long)st.entries, (unsigned long long)st.blocks, st.kernel, st.depth);
        if (sha1chunk_pv_pending(g_pv)) fatal("results pending at the end");
        sha1chunk_pv_destroy(g_pv);
    }
    if (g_vq) {
        if (sha1chunk_vq_pending(g_vq)) fatal("results pending at the end");
        sha1chunk_vq_destroy(g_vq);
    }
#endif
    printf("RSM COUNTS delivered=%lu copied_dups=%lu strays=%lu stability_writes=%lu ring_full=%lu syncs=%lu\n",
           g_delivered, g_copied_dups, g_strays, g_stab, g_ring_full, g_syncs);
    return 0;
}
