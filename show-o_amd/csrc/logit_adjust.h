// Logit adjustment of the mmu decode (logit_adjust.hip; include/showo_hip.h, "Logit adjustment"): repetition penalty over a bitmap
// of seen tokens and an additive bias row, written to a second row so that the raw logits stay what the head wrote.
#pragma once
#include "common.h"

namespace showo {

// What a decode loop carries for its adjust launch: fixed for the duration of one call (the launch is a node of the captured step).
struct LogitAdjust {
    uint32_t* seen;            // bitmap [rows, seen_ld]
    int64_t seen_ld;
    const float* penalty;      // host [rows]
    const float* const* bias;  // host [rows] of device rows fp32 [V], entries may be NULL; NULL: no row has one
    float* ws;                 // device fp32 [rows, V]: what the pick reads
};

// every penalty finite and > 0, seen_ld covers V, the pointers are there: error 1 otherwise (nothing is launched)
int logits_adjust_check(int nrows, int V, const uint32_t* seen, int64_t seen_ld, const float* penalty, const char* who);

// showo_logits_adjust with a strided `active` (ints, one every active_stride; NULL: every row is active)
int logits_adjust_launch(const float* logits, int64_t ld, int nrows, int V, uint32_t* seen, int64_t seen_ld, const int64_t* mark,
                         const float* penalty, const float* const* bias, const int* active, int active_stride, float* out, int64_t ld_out,
                         hipStream_t s);

}  // namespace showo
