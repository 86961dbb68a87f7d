// Functions one translation unit of libmorb_hip.so defines for the others (the handle structs themselves are in handles.h).
// HIDDEN visibility so that the library exports exactly what include/morb_hip.h declares (tests/test_oracle_cpu.py compares
// `nm -D` with the header).
#pragma once
#include <cstddef>

#include "handles.h"

#define MORB_INTERNAL __attribute__((visibility("hidden")))
extern "C" {
// matcher.hip
MORB_INTERNAL int morb_matcher_const(morb_matcher*, morb_matcher::ConstTable table, const void* host, size_t bytes, void** d_out, void* stream);
MORB_INTERNAL int morb_bow_sort_images(morb_matcher* m, int nimg, const int* d_node, const int* d_count, int cap, unsigned long long** d_sorted,
                                       void* stream);
// optimizer.hip
MORB_INTERNAL int morb_optimizer_lm_words(morb_optimizer*, int** host, int** dev);   // 16 pinned, device-mapped ints (LM state mirror), made on first use
}
