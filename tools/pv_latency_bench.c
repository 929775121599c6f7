/*
 * pv_latency_bench -- what progressive verification (sha1chunk_pv,
 * include/sha1chunk.h) buys the peer's receive path: the time from a
 * chunk's last packet to its verdict.
 *
 *   run A   one 512 KiB chunk fed in its 354 DATA packets (353 x 1484 +
 *           436), the hashing allowed to keep up (each packet's blocks
 *           confirmed before the next is fed); time from the final advance
 *           to the result by non-blocking polls.  Also the time each packet
 *           took to be confirmed (launch + ~23 blocks read over PCIe), which
 *           is where the prefetch depth shows.
 *   run A'  the same chunk fed without waiting (the host outruns the lane):
 *           the verdict then trails the last packet by the backlog.
 *   run B   the same chunk through sha1chunk_vq_submit on a lone-chunk
 *           queue: the existing path, the reference for the time.
 *   run C   4, 16, 64 and 256 concurrent sessions advanced round-robin one
 *           packet at a time: aggregate bytes/s, fed two ways -- "per_call",
 *           one sha1chunk_pv_advance per session and packet, and "burst", one
 *           sha1chunk_burst_advance per round-robin round -- with the kernel
 *           choice and the launches issued (sha1chunk_progress_stats).
 *
 * One JSON line per run on stdout.  SHA1CHUNK_PV_DEPTH (2, 4, 8) selects the
 * lane kernel's prefetch depth and SHA1CHUNK_PV_KERNEL (auto, lane, shared)
 * the kernel, for the A/Bs of DESIGN.md section 6.
 *   usage: pv_latency_bench [chunks (default 24)]
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../include/sha1chunk.h"

#define LEN SHA1CHUNK_CHUNK_LEN
#define PKT 1484u
#define MAXN 256

static double now_us(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

static int cmp_d(const void *a, const void *b) {
    const double x = *(const double *)a, y = *(const double *)b;
    return x < y ? -1 : x > y;
}

static void die(const char *what) {
    fprintf(stderr, "pv_latency_bench: %s: %s\n", what, sha1chunk_last_error());
    exit(1);
}

static void stats_line(const char *run, const char *depth, double *v, int n, const char *extra) {
    qsort(v, (size_t)n, sizeof *v, cmp_d);
    printf("{\"run\": \"%s\", \"depth\": %s, \"chunk_bytes\": %d, \"chunks\": %d, \"median_us\": %.1f, "
           "\"min_us\": %.1f, \"max_us\": %.1f%s}\n",
           run, depth, LEN, n, v[n / 2], v[0], v[n - 1], extra);
    fflush(stdout);
}

/* One chunk through the progressive verifier; returns final advance -> result
 * in us.  keep_up: wait for each packet's blocks before the next packet;
 * *per_packet (if not NULL) receives the mean confirmation time of a packet. */
static double pv_chunk(sha1chunk_pv *p, const uint8_t *chunk, const uint8_t *dig, uint64_t tag, int keep_up,
                       double *per_packet) {
    uint8_t *buf = NULL;
    while (!(buf = (uint8_t *)sha1chunk_pv_open(p, LEN, dig, tag)))
        if (!strstr(sha1chunk_last_error(), "in use")) die("open");
    uint32_t mark = 0, h = 0;
    double waited = 0;
    int packets = 0;
    while (mark + PKT < LEN) {
        memcpy(buf + mark, chunk + mark, PKT);
        mark += PKT;
        const double t0 = now_us();
        if (sha1chunk_pv_advance(p, buf, mark)) die("advance");
        if (!keep_up) continue;
        do {
            if (sha1chunk_pv_hashed(p, buf, &h)) die("hashed");
        } while (h < (mark & ~63u));
        waited += now_us() - t0;
        ++packets;
    }
    memcpy(buf + mark, chunk + mark, LEN - mark);
    uint64_t t;
    uint8_t m;
    const double t0 = now_us();
    if (sha1chunk_pv_advance(p, buf, LEN)) die("final advance");
    long n;
    while ((n = sha1chunk_pv_poll(p, &t, &m, NULL, 1, 0)) == 0) {
    }
    const double t1 = now_us();
    if (n != 1 || t != tag || m != 0) die("wrong result");
    if (sha1chunk_pv_close(p, buf)) die("close");
    if (per_packet) *per_packet = packets ? waited / packets : 0;
    return t1 - t0;
}

static double vq_chunk(sha1chunk_vq *q, const uint8_t *chunk, const uint8_t *dig, uint64_t tag) {
    uint64_t t;
    uint8_t m;
    const double t0 = now_us();
    if (sha1chunk_vq_submit(q, chunk, LEN, dig, tag)) die("vq_submit");
    long n;
    while ((n = sha1chunk_vq_poll(q, &t, &m, 1, 0)) == 0) {
    }
    const double t1 = now_us();
    if (n != 1 || t != tag || m != 0) die("wrong vq result");
    return t1 - t0;
}

static void run_c(const uint8_t *chunk, const uint8_t *dig, const char *depth, int S, int burst) {
    static const char *const kernels[] = {"auto", "lane", "shared"};
    sha1chunk_pv *p = sha1chunk_pv_create((size_t)S, LEN);
    if (!p) die("create (run C)");
    static uint8_t *buf[MAXN];
    static uint32_t marks[MAXN];
    sha1chunk_progress_stats_t st0, st1;
    for (int pass = 0; pass < 2; ++pass) { /* pass 0 warms (code object, page faults) */
        for (int s = 0; s < S; ++s)
            while (!(buf[s] = (uint8_t *)sha1chunk_pv_open(p, LEN, dig, (uint64_t)s)))
                if (!strstr(sha1chunk_last_error(), "in use")) die("open (run C)");
        if (sha1chunk_progress_stats(p, &st0, sizeof st0)) die("stats (run C)");
        const double t0 = now_us();
        for (uint32_t mark = 0; mark < LEN;) {
            const uint32_t step = LEN - mark < PKT ? LEN - mark : PKT;
            for (int s = 0; s < S; ++s) {
                memcpy(buf[s] + mark, chunk + mark, step);
                marks[s] = mark + step;
                if (!burst && sha1chunk_pv_advance(p, buf[s], mark + step)) die("advance (run C)");
            }
            if (burst && sha1chunk_burst_advance(p, (void *const *)buf, marks, (size_t)S, NULL))
                die("burst advance (run C)");
            mark += step;
        }
        const double t_fed = now_us();
        static uint64_t tags[MAXN];
        static uint8_t mis[MAXN];
        long got = 0;
        while (got < S) {
            const long n = sha1chunk_pv_poll(p, tags, mis, NULL, MAXN, 1);
            if (n < 0) die("poll (run C)");
            for (long i = 0; i < n; ++i)
                if (mis[i]) die("mismatch (run C)");
            got += n;
        }
        const double t1 = now_us();
        for (int s = 0; s < S; ++s) sha1chunk_pv_close(p, buf[s]);
        if (sha1chunk_progress_stats(p, &st1, sizeof st1)) die("stats (run C)");
        if (pass == 1) {
            printf("{\"run\": \"C\", \"depth\": %s, \"kernel\": \"%s\", \"feed\": \"%s\", \"sessions\": %d, "
                   "\"chunk_bytes\": %d, \"feed_ms\": %.3f, \"total_ms\": %.3f, \"tail_after_last_packet_ms\": %.3f, "
                   "\"bytes_per_s\": %.4g, \"launches\": %llu, \"launches_shared\": %llu, \"entries\": %llu}\n",
                   depth, kernels[st1.kernel < 3 ? st1.kernel : 0], burst ? "burst" : "per_call", S, LEN,
                   (t_fed - t0) * 1e-3, (t1 - t0) * 1e-3, (t1 - t_fed) * 1e-3, (double)S * LEN / ((t1 - t0) * 1e-6),
                   (unsigned long long)(st1.launches - st0.launches),
                   (unsigned long long)(st1.launches_shared - st0.launches_shared),
                   (unsigned long long)(st1.entries - st0.entries));
            fflush(stdout);
        }
    }
    sha1chunk_pv_destroy(p); /* its pv_stats line (both passes) goes to stderr */
}

int main(int argc, char **argv) {
    int N = argc > 1 ? atoi(argv[1]) : 24;
    if (N < 20) N = 20;
    if (N > MAXN) N = MAXN;
    setenv("SHA1CHUNK_PV_STATS", "1", 0);
    const char *depth = getenv("SHA1CHUNK_PV_DEPTH");
    if (!depth || !*depth) depth = "4";
    uint8_t *chunk = (uint8_t *)malloc(LEN);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < LEN; ++i) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        chunk[i] = (uint8_t)(x >> 32);
    }
    uint8_t dig[20];
    if (sha1chunk_digest(chunk, LEN, dig)) die("digest");

    static double v[MAXN], pp[MAXN];
    sha1chunk_pv *p = sha1chunk_pv_create(2, LEN);
    if (!p) die("create");
    pv_chunk(p, chunk, dig, 0, 1, NULL); /* warm-up */
    for (int i = 0; i < N; ++i) v[i] = pv_chunk(p, chunk, dig, 1 + (uint64_t)i, 1, &pp[i]);
    qsort(pp, (size_t)N, sizeof *pp, cmp_d);
    char extra[160];
    snprintf(extra, sizeof extra, ", \"packet_confirm_us_median\": %.1f, \"packet_confirm_us_min\": %.1f, "
             "\"packet_confirm_us_max\": %.1f", pp[N / 2], pp[0], pp[N - 1]);
    stats_line("A_keep_up", depth, v, N, extra);
    for (int i = 0; i < N; ++i) v[i] = pv_chunk(p, chunk, dig, 1000 + (uint64_t)i, 0, NULL);
    stats_line("A_burst_no_wait", depth, v, N, "");
    sha1chunk_pv_destroy(p);

    sha1chunk_vq *q = sha1chunk_vq_create(256, LEN);
    if (!q) die("vq_create");
    vq_chunk(q, chunk, dig, 0);
    for (int i = 0; i < N; ++i) v[i] = vq_chunk(q, chunk, dig, 1 + (uint64_t)i);
    stats_line("B_vq_submit_lone_chunk", depth, v, N, "");
    sha1chunk_vq_destroy(q);

    static const int counts[] = {4, 16, 64, 256};
    for (size_t i = 0; i < sizeof counts / sizeof *counts; ++i)
        for (int burst = 0; burst < 2; ++burst) run_c(chunk, dig, depth, counts[i], burst);
    free(chunk);
    return 0;
}
