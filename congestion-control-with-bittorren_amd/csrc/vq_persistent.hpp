// vq_persistent.hpp -- the persistent verify queue (vq_persistent.hip) as
// vq.hip sees it: an opaque Pvq behind the queue's lock.  Every call but
// pvq_create and pvq_destroy is made with that lock (`mu`) held; a call that
// has to wait for the device drops it while it sleeps.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <mutex>

#include "sha1_runtime_internal.h"

namespace s1rt {
struct Pvq;

// cus: the drain's workgroups, taken from D's budget (drain_cus_take) and
// given back by pvq_destroy.  Null on failure (the thread's error text set).
Pvq* pvq_create(Device* D, size_t batch, uint32_t max_chunk_len, int cus, std::mutex* mu);
void pvq_destroy(Pvq* P);
uint32_t pvq_max_len(const Pvq* P);
size_t pvq_pending(const Pvq* P);
int pvq_submit(Pvq* P, const void* chunk, uint32_t len, const uint8_t expected[20], uint64_t tag);
void* pvq_reserve(Pvq* P, uint32_t len);
int pvq_commit(Pvq* P, void* buf, uint32_t len, const uint8_t expected[20], uint64_t tag);
int pvq_release(Pvq* P, void* buf);
int pvq_publish(Pvq* P);  // flush: the open group goes out
long pvq_poll(Pvq* P, uint64_t* tags, uint8_t* mismatch, size_t max, int wait);
// The queue's counters, as fields of the SHA1CHUNK_VQ_STATS JSON line.
void pvq_print_stats(const Pvq* P, FILE* f);
}  // namespace s1rt
