// Sequence rules of the mmu decode (seq_rules.hip; include/showo_hip.h, "Sequence rules"): no-repeat n-grams, multi-token bad words
// and a minimum length, as -inf stores into the row the pick reads, computed from a token history that lives on the device.
#pragma once
#include "common.h"
#include "../../include/showo_hip.h"

namespace showo {

constexpr int SEQ_NGRAM_MAX = 16;  // largest no_repeat_ngram_size served (the tail's n - 1 tokens live in LDS)

// the pointers are there, hist_ld >= 1, every ngram in [0, SEQ_NGRAM_MAX], ctx_len / min_new >= 0: error 1 otherwise (nothing is launched)
int seq_rules_check(int nrows, const showo_seq_rules* rules, const char* who);

// showo_seq_ban with a strided `active` (ints, one every active_stride; NULL: every row is active)
int seq_ban_launch(float* rows, int64_t ld, int nrows, int V, const showo_seq_rules* rules, const int64_t* mark, const int* active,
                   int active_stride, hipStream_t s);

}  // namespace showo
