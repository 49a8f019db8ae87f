// scan.h - the launches of the band scan's kernels (scan.hip; include/psdr.h: psdr_scan_batch): behind a batch's passes and
// pyramid tails on the side stream, beside the waterfall gather.  They read the batch's int8 pyramid and nothing else of the
// context, and write the scan's own buffers only; no other kernel knows of them.  Every step with arithmetic is scanplan.h's,
// shared with the host; scan.hip is the lanes' side of it: loads, ballots, the block scan, atomics, stores.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"
#include "scanplan.h"

namespace psdr {

// k_scan_trace: one lane per `per` adjacent values of the level, the loop over the batch's frames in order
struct ScanTraceArgs {
    const int8_t *src;  // tiled: the batch's records; level-major: the level's first byte in frame 0
    size_t stride;      // bytes from a frame to the next
    uint16_t *trace;
    size_t lanes;       // n / per
    RecMap map;         // tiled: where record g sits
    int rec_bytes, loff, tiled;
    int nframes, fresh, shift;
};
// k_scan_floor, k_scan_hot, k_scan_mark, k_scan_emit: the evaluation
struct ScanEvalArgs {
    const uint16_t *trace;
    uint32_t *Q, *F;
    uint64_t *hot, *starts;
    uint32_t *base;
    ScanRun *list;
    ScanHead *head;
    int G, threshold, gap;
    unsigned words;
};

constexpr int SCAN_MARK_THREADS = 1024;

// each on stream `s`; per: 16, 8, 4, 2 or 1 (scanplan.h: scan_launch)
hipError_t scan_trace_launch(const ScanTraceArgs &a, int per, unsigned blocks, hipStream_t s);
hipError_t scan_floor_launch(const ScanEvalArgs &a, unsigned blocks, hipStream_t s);
hipError_t scan_hot_launch(const ScanEvalArgs &a, unsigned blocks, hipStream_t s);
hipError_t scan_mark_launch(const ScanEvalArgs &a, hipStream_t s);
hipError_t scan_emit_launch(const ScanEvalArgs &a, unsigned blocks, hipStream_t s);

}  // namespace psdr
