// Beam search on the device ("Beam search"): the records and launches that beam.hip gives the batched decode loop
// (decode_batch.hip showo_engine_batch_decode_beam).  The layouts are part of the C ABI (include/showo_hip.h).
#pragma once
#include "common.h"

namespace showo {

constexpr int BEAM_MAX = 8;          // beams (the <= 8-slot batched step serves them)
constexpr int BEAM_STATE_HEAD = 64;  // 32-bit words in front of the length-penalty table of a state block

// word offsets inside a state block (int32 [BEAM_STATE_HEAD + max_new + 1], device)
enum BeamStateWord {
    BS_T = 0,        // tokens every live beam has generated so far
    BS_DONE = 1,     // the search is over: every later step idles
    BS_NHYP = 2,     // finished hypotheses in the table
    BS_WORST = 3,    // fp32: the worst kept final score once the table is full, else -inf
    BS_MAXNEW = 4,   // max_new_tokens of the search
    BS_B = 5,        // beams
    BS_ORDER = 6,    // hypotheses ever inserted (the `order` of the next one)
    BS_CUM = 8,      // fp32 [8]: cumulative score of every live beam
    BS_PARENT = 16,  // int32 [8]: the parent map of the step just taken (identity while idle): what showo_kv_permute_rows reads
    BS_TOK = 32,     // int64 [8]: the token every live beam feeds next
    // word BEAM_STATE_HEAD + len: fp32 len ** length_penalty, len = 1 .. max_new (written by the host: the divisor of a final score)
};

struct BeamCand {  // one of the 2B best continuations, best first
    float score;
    int32_t beam;
    int32_t token;
};
struct BeamHyp {  // a finished hypothesis; the table is kept sorted by (final descending, order ascending)
    int32_t step;  // trace row of its last token
    int32_t beam;  // kind 0: the live beam of row step - 1 it continues with <eot>; kind 1: the live beam of row `step` it is
    int32_t kind;  // 0: ended on <eot>; 1: a live beam at max_new_tokens
    float final;   // sumlp / len ** length_penalty
    int32_t len;   // generated tokens, the <eot> included
    float sumlp;
    int32_t order;
    float lp;      // log-probability of its last token (kind 0: of the <eot>, which no trace row holds)
};
static_assert(sizeof(BeamCand) == 12 && sizeof(BeamHyp) == 32, "ABI layouts");

struct BeamSeamArgs {
    const float* logits;  // [rows, V] with leading dimension ld: the rows the candidates index (1 row in the first step, else B)
    int64_t ld;
    int V;
    const float* norm;     // [rows, 2] of the selection
    const BeamCand* cand;  // [2B]
    int B;
    int64_t eot;  // < 0: nothing finishes early
    int early;
    int first;  // the step on the prefill's row: positions do not advance
    int32_t* state;
    int32_t *tr_parent, *tr_token;  // [max_new, B]
    float *tr_cum, *tr_lp;
    BeamHyp* hyp;  // [B]
    int* pos;
    int lim;
    const float* table;  // embedding [V, H]
    float* x;            // [B, H] rows of the next step
    int H;
    const int32_t* last_iv;
    const int* L0;
    int32_t* iv;
};

// norm [nb, 2], cand [2B], ws fp32 [nb, 2B, 2]; two launches
int beam_select_launch(const float* logits, int64_t ld, int nb, int V, const float* cum, int B, float* norm, BeamCand* cand, float* ws,
                       hipStream_t s);
int beam_seam_launch(const BeamSeamArgs& a, hipStream_t s);
// stage pitch (rows / columns) of a staging buffer that serves spans of up to `span` rows
inline int64_t kv_permute_pitch(int span) { return ((int64_t)(span + 7) / 8 + 1) * 8; }

}  // namespace showo
