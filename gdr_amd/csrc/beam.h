// The beam and greedy bookkeeping of a docid decode (beam.hip), as far as the model step (decode.hip) needs it: the step's logits go
// into BeamBufs::logits, the step's input tokens and ancestor rows come out of cur_tok / kv_rows.  Nothing here knows a model.
#pragma once
#include "common.h"

namespace gdr {

constexpr int PAD_ID = 0, EOS_ID = 1, START_ID = 0;
constexpr int MAXLEN_CAP = 32;

struct BeamBufs {
  int32_t* seq[2];      // [rows][maxlen] token history, double buffered
  float* beam_scores;   // [rows]
  int64_t* cur_tok;     // [rows] last token of each row (embedding input of the step)
  int32_t* parent;      // [rows] row of the previous step that each row extends
  int32_t* anc[2];      // [rows][maxlen] row whose cache slot holds position p of this row's prefix
  int32_t* kv_rows;     // [rows][s+1] absolute cache row = p*rows + anc
  int32_t* node[2];     // [rows] trie node reached by the row's prefix (-1: left the tree), double buffered
  int32_t* miss_rows;   // [rows] prefix-table mode: rows whose prefix has no table entry, compacted (ascending)
  int32_t* miss_index;  // [rows] inverse: position of a row in miss_rows, or -1 when its prefix hit the table
  int32_t* kv_rows_c;   // [rows][maxlen] kv_rows of the compacted rows
  int64_t* n_miss;      // [1] number of compacted rows (read by the kernels of the adaptor chain)
  float* logits;        // [rows][V+1] unmasked-column logits of the step
  float* cand_score;    // [B][2R]
  int32_t* cand_idx;    // [B][2R]  beam*Vd + token
  double* hyp_score;    // [B][R+1]
  int32_t* hyp_len;     // [B][R+1]
  int32_t* hyp_tok;     // [B][R+1][maxlen]
  int32_t* hyp_seq;     // [B][R+1] insertion number of each live hypothesis (list order of the reference's self.beams)
  int32_t* hyp_next;    // [B] next insertion number
  int32_t* hyp_cnt;     // [B]
  double* hyp_worst;    // [B]
  int32_t* done;        // [B]
  int32_t* n_done;      // [1] queries whose beam search is done (generation_utils.py:827-829)
  int32_t* live;        // [1] 1 until n_done reaches B: the linears and the miss-row chain of later steps look at it
  float* lse;                     // chunked select only: [rows][2] every beam row's (max, log-sum-exp) of the step
  unsigned long long* part[2];    // chunked select only: [B][lists][2R] sorted partial lists of keys, ping-pong over the merge rounds
  const int32_t* live_gate;  // = live when the call may skip the steps behind the last query's end (no per-step trace wanted), else
                             // null: the attention / reduction / head / beam kernels of such a step exit at once through it
  int32_t* all_done_host;  // host-mapped word (may be null): receives `done_epoch` when n_done reaches B
  int32_t done_epoch;
};

struct BeamDims {
  int B, R, V, Vd, maxlen, nret;
  double lp;
  // docid trie: child[node*V + c] = next node or -1 for the digit c of the node's depth.  trie_child alone = rows only
  // TRACK the node their prefix reaches (prefix-table mode); with trie_eos (eos_ok[node] = 1 if EOS is a child) the
  // trie also CONSTRAINS the beams (generation_utils_previous.py:714-729).  Both null = the shipped behaviour.
  const int32_t* trie_child;
  const int32_t* trie_eos;
  int trie_nodes;
};

// the next region of a workspace: `bytes` at offset `o`, which moves on to the next multiple of 256
static inline size_t carve(size_t& o, size_t bytes) {
  const size_t at = o;
  o += align_up(bytes, 256);
  return at;
}

// bytes of the beam workspace; with `base` (and bb) the regions' pointers are filled in
size_t beam_layout(const BeamDims& bd, char* base, BeamBufs* bb);

int check_beam_dims(const BeamDims& bd, int max_length);
int check_greedy_dims(const BeamDims& bd, int max_length);
int check_forced_dims(const BeamDims& bd, int max_length);

// num_beams >= 2: once per call; after bb.logits holds the logits of position `pos`; after the last step
int beam_begin(const BeamBufs& bb, const BeamDims& bd, hipStream_t stream, bool dedup0 = false);
int beam_step(const BeamBufs& bb, const BeamDims& bd, int pos, int cur, float* step_scores, int32_t* step_tokens, hipStream_t stream,
              bool bcast = false);
int beam_end(const BeamBufs& bb, const BeamDims& bd, int max_length, int cur, int64_t* out_ids, int32_t* out_len, double* out_scores,
             hipStream_t stream);
// num_beams = 1: out_ids / out_len are written as the steps go, there is no end
int greedy_begin(const BeamBufs& bb, const BeamDims& bd, int64_t* out_ids, int32_t* out_len, double* out_scores, hipStream_t stream);
int greedy_step(const BeamBufs& bb, const BeamDims& bd, int pos, int cur, int64_t* out_ids, int32_t* out_len, hipStream_t stream);
// given tokens (teacher forcing, gdr_t5_generate's score mode): `ids` [rows][maxlen] are read, never written.  Once per call; after
// bb.logits holds the logits of position `pos` (none behind the last position, pos = maxlen - 1) and `hl` [rows][d] its last hidden
// states, which go into `planes` [maxlen + 2][rows][d] when that is given; after the last position
int forced_begin(const BeamBufs& bb, const BeamDims& bd, const int64_t* ids, hipStream_t stream);
int forced_step(const BeamBufs& bb, const BeamDims& bd, int pos, const int64_t* ids, const float* hl, int d, float* planes,
                hipStream_t stream);
int forced_end(const BeamBufs& bb, const BeamDims& bd, const int64_t* ids, int d, float* planes, double* out_scores, hipStream_t stream);

}  // namespace gdr
