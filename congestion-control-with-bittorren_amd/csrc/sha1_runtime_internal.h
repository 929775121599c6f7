// sha1_runtime_internal.h -- what the backend's other translation units
// (sha1_pv.hip) share with sha1_runtime.hip: the thread's error text and
// device, and the verify queue's pinned-memory kind and stream helper.  Internal to
// libsha1chunk_hip.so (hidden symbols).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sha1chunk.h"

#define S1RT_HIDDEN __attribute__((visibility("hidden")))

namespace s1rt {
// Sets the calling thread's error text (s1be_last_error) and returns code.
S1RT_HIDDEN int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// The calling thread's device (s1be_set_device), initialised and made
// current: its HIP id and CU count.  0 or a negative error.
S1RT_HIDDEN int acquire_device(int* hip_id, int* cus);
// The hipHostMalloc kind of pinned memory the device reads over PCIe while
// the host writes it, as the persistent verify queue's ring is allocated:
// SHA1CHUNK_VQ_RING_MEM ("uncached", the default, or "coherent").
S1RT_HIDDEN unsigned pinned_ring_flags();
// A stream at the verify queues' priority (SHA1CHUNK_VQ_PRIO).  0 or -1.
S1RT_HIDDEN int stream_create(hipStream_t* s);
}  // namespace s1rt

// `fail` is the including file's: sha1_runtime.hip's own, s1rt::fail elsewhere.
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(SHA1CHUNK_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                  \
    } while (0)
