// Step-input packer: lays out everything one engine step uploads to the GPU
// (token ids, positions, KV slots, prefill tiles, padded block tables, ...)
// in ONE caller-provided host buffer, so the step needs a single
// host-to-device copy. Plain C++ over raw pointers: no torch, no pybind, no
// allocation. Values and dtypes match ModelRunner.prepare() section for
// section (tests/test_step_pack.py holds the two against each other).
//
// Sequences come in the order prepare() uses: prefill chunks first, then
// decode rows (one token each).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace ps {

enum StepPackStatus : int {
  STEP_PACK_OK = 0,
  // capacity < layout.total_bytes; nothing was written, grow and retry
  STEP_PACK_TOO_SMALL = 1,
  // a prefill chunk holds a -1 placeholder (a preempted sequence readmitted
  // for recompute before its last token resolved): the sync path must run
  STEP_PACK_PREFILL_PLACEHOLDER = 2,
  // a decode row holds a placeholder but names no row of the previous
  // step's sampled tensor
  STEP_PACK_DECODE_UNRESOLVED = 3,
  // inconsistent descriptors (order, sizes, a position past its block table)
  STEP_PACK_BAD_INPUT = 4,
};

struct StepPackIn {
  int64_t num_seqs;
  const int32_t* start;        // [num_seqs] first position of the chunk
  const int32_t* num_tokens;   // [num_seqs] rows of the chunk (decode: 1)
  const uint8_t* is_decode;    // [num_seqs] prefills first, then decodes
  const uint8_t* sample_last;  // [num_seqs] prefill: last row is sampled
                               // (decode rows are always sampled)
  const int32_t* prev_row;     // [num_seqs] decode placeholder: its row in
                               // the previous step's sampled tensor, else <0
  const int64_t* token_ids;    // flat, sum(num_tokens); -1 = placeholder
  int64_t num_token_ids;       // entries in token_ids
  const int32_t* tables;       // flat block tables, unpadded
  int64_t num_table_entries;   // entries in tables
  const int64_t* table_off;    // [num_seqs + 1] offsets into tables
  int32_t block_size;
  int32_t tile_rows;           // ops.prefill_tile_rows
};

// Counts and byte offsets (from the start of the buffer) of every section.
// The same struct is written at offset 0 of the packed buffer.
struct StepPackLayout {
  int64_t total_bytes;
  int64_t num_tokens;          // T
  int64_t num_prefill_tokens;  // Tp
  int64_t num_prefill_seqs;    // Sp
  int64_t num_decode_seqs;     // Sd
  int64_t num_tiles;           // NT
  int64_t max_bt;              // common padded block-table width
  int64_t num_sample_rows;     // R
  int64_t num_placeholders;    // decode rows with prev_row >= 0
  int64_t off_tokens;          // int64 [T]
  int64_t off_positions;       // int32 [T]
  int64_t off_slot_mapping;    // int64 [T]
  int64_t off_prefill_token_seq;     // int32 [Tp]
  int64_t off_prefill_token_pos;     // int32 [Tp]
  int64_t off_prefill_tiles;         // int32 [NT, 4]
  int64_t off_prefill_block_tables;  // int32 [Sp, max_bt]
  int64_t off_decode_block_tables;   // int32 [Sd, max_bt]
  int64_t off_decode_seq_lens;       // int32 [Sd]
  int64_t off_sample_rows;           // int64 [R]
  int64_t off_prev_row;              // int32 [T]
};

constexpr int64_t kStepPackAlign = 16;
constexpr int64_t kStepPackFields = sizeof(StepPackLayout) / sizeof(int64_t);

namespace step_pack_detail {

inline int64_t align_up(int64_t v) {
  return (v + kStepPackAlign - 1) / kStepPackAlign * kStepPackAlign;
}

// sizes are bounded so that every product below stays far from overflow
constexpr int64_t kMaxCount = int64_t(1) << 28;

}  // namespace step_pack_detail

// Validates the descriptors, computes the layout, and, if `capacity` bytes
// suffice, fills `buf`. On any status other than STEP_PACK_OK nothing is
// written to `buf`; `layout` is valid for OK and TOO_SMALL. Never writes
// outside [buf, buf + capacity).
inline int step_pack(const StepPackIn& in, void* buf, int64_t capacity,
                     StepPackLayout* layout) {
  using namespace step_pack_detail;
  StepPackLayout L;
  std::memset(&L, 0, sizeof(L));
  *layout = L;
  const int64_t n = in.num_seqs;
  const int64_t bs = in.block_size;
  const int64_t tile = in.tile_rows;
  if (n < 0 || n > kMaxCount || bs <= 0 || tile <= 0) {
    return STEP_PACK_BAD_INPUT;
  }

  // ---- pass 1: validate and count; no writes --------------------------
  int status = STEP_PACK_OK;
  bool seen_decode = false;
  int64_t tok = 0;
  L.max_bt = n ? 0 : 1;
  for (int64_t s = 0; s < n; ++s) {
    const int64_t cnt = in.num_tokens[s];
    const int64_t start = in.start[s];
    const int64_t bt_len = in.table_off[s + 1] - in.table_off[s];
    if (cnt < 0 || start < 0 || bt_len < 0 || bt_len > kMaxCount ||
        in.table_off[s] < 0 || in.table_off[s + 1] > in.num_table_entries ||
        start + cnt > INT32_MAX || tok + cnt > in.num_token_ids) {
      return STEP_PACK_BAD_INPUT;
    }
    const bool dec = in.is_decode[s] != 0;
    if (dec) {
      seen_decode = true;
      if (cnt != 1) return STEP_PACK_BAD_INPUT;
    } else if (seen_decode) {
      return STEP_PACK_BAD_INPUT;  // prefills must come first
    }
    // every position of the chunk indexes its block table
    if (cnt > 0 && (start + cnt - 1) / bs >= bt_len) {
      return STEP_PACK_BAD_INPUT;
    }
    if (bt_len > L.max_bt) L.max_bt = bt_len;
    for (int64_t j = 0; j < cnt; ++j) {
      if (in.token_ids[tok + j] >= 0) continue;
      if (!dec) {
        if (status == STEP_PACK_OK) status = STEP_PACK_PREFILL_PLACEHOLDER;
      } else if (in.prev_row[s] < 0) {
        if (status == STEP_PACK_OK) status = STEP_PACK_DECODE_UNRESOLVED;
      } else {
        L.num_placeholders += 1;
      }
    }
    tok += cnt;
    if (tok > kMaxCount) return STEP_PACK_BAD_INPUT;
    if (dec) {
      L.num_decode_seqs += 1;
      L.num_sample_rows += 1;
    } else {
      L.num_prefill_seqs += 1;
      L.num_prefill_tokens += cnt;
      L.num_tiles += (cnt + tile - 1) / tile;
      if (in.sample_last[s] && cnt > 0) L.num_sample_rows += 1;
    }
  }
  if (status != STEP_PACK_OK) return status;
  L.num_tokens = tok;
  if (L.max_bt * (L.num_prefill_seqs + L.num_decode_seqs) > kMaxCount * 8) {
    return STEP_PACK_BAD_INPUT;
  }

  int64_t off = align_up((int64_t)sizeof(StepPackLayout));
  auto section = [&off](int64_t count, int64_t elem) {
    const int64_t at = off;
    off = align_up(off + count * elem);
    return at;
  };
  L.off_tokens = section(L.num_tokens, 8);
  L.off_positions = section(L.num_tokens, 4);
  L.off_slot_mapping = section(L.num_tokens, 8);
  L.off_prefill_token_seq = section(L.num_prefill_tokens, 4);
  L.off_prefill_token_pos = section(L.num_prefill_tokens, 4);
  L.off_prefill_tiles = section(L.num_tiles * 4, 4);
  L.off_prefill_block_tables = section(L.num_prefill_seqs * L.max_bt, 4);
  L.off_decode_block_tables = section(L.num_decode_seqs * L.max_bt, 4);
  L.off_decode_seq_lens = section(L.num_decode_seqs, 4);
  L.off_sample_rows = section(L.num_sample_rows, 8);
  L.off_prev_row = section(L.num_tokens, 4);
  L.total_bytes = off;
  *layout = L;
  if (buf == nullptr || capacity < L.total_bytes) return STEP_PACK_TOO_SMALL;
  if (reinterpret_cast<uintptr_t>(buf) % kStepPackAlign != 0) {
    return STEP_PACK_BAD_INPUT;  // the sections hold int64
  }

  // ---- pass 2: fill ---------------------------------------------------
  char* base = static_cast<char*>(buf);
  // padding between sections and the block tables' tails are zero
  std::memset(base, 0, (size_t)L.total_bytes);
  std::memcpy(base, &L, sizeof(L));
  auto* tokens = reinterpret_cast<int64_t*>(base + L.off_tokens);
  auto* positions = reinterpret_cast<int32_t*>(base + L.off_positions);
  auto* slots = reinterpret_cast<int64_t*>(base + L.off_slot_mapping);
  auto* p_seq = reinterpret_cast<int32_t*>(base + L.off_prefill_token_seq);
  auto* p_pos = reinterpret_cast<int32_t*>(base + L.off_prefill_token_pos);
  auto* tiles = reinterpret_cast<int32_t*>(base + L.off_prefill_tiles);
  auto* p_bt = reinterpret_cast<int32_t*>(base + L.off_prefill_block_tables);
  auto* d_bt = reinterpret_cast<int32_t*>(base + L.off_decode_block_tables);
  auto* d_len = reinterpret_cast<int32_t*>(base + L.off_decode_seq_lens);
  auto* rows = reinterpret_cast<int64_t*>(base + L.off_sample_rows);
  auto* prev = reinterpret_cast<int32_t*>(base + L.off_prev_row);

  int64_t t = 0, p_row = 0, d_row = 0, n_tiles = 0, n_rows = 0;
  for (int64_t s = 0; s < n; ++s) {
    const int64_t cnt = in.num_tokens[s];
    const int64_t start = in.start[s];
    const int32_t* bt = in.tables + in.table_off[s];
    const int64_t bt_len = in.table_off[s + 1] - in.table_off[s];
    const bool dec = in.is_decode[s] != 0;
    int32_t* bt_out = dec ? d_bt + d_row * L.max_bt : p_bt + p_row * L.max_bt;
    if (bt_len) std::memcpy(bt_out, bt, (size_t)bt_len * sizeof(int32_t));
    if (!dec) {
      for (int64_t t0 = 0; t0 < cnt; t0 += tile) {
        int32_t* ti = tiles + 4 * n_tiles++;
        ti[0] = (int32_t)p_row;
        ti[1] = (int32_t)(t + t0);
        ti[2] = (int32_t)(start + t0);
        ti[3] = (int32_t)(cnt - t0 < tile ? cnt - t0 : tile);
      }
    }
    for (int64_t j = 0; j < cnt; ++j, ++t) {
      const int64_t pos = start + j;
      tokens[t] = in.token_ids[t];
      positions[t] = (int32_t)pos;
      slots[t] = (int64_t)bt[pos / bs] * bs + pos % bs;
      prev[t] = (dec && in.token_ids[t] < 0) ? in.prev_row[s] : -1;
      if (!dec) {
        p_seq[t] = (int32_t)p_row;
        p_pos[t] = (int32_t)pos;
      }
    }
    if (dec) {
      d_len[d_row++] = (int32_t)(start + 1);
      rows[n_rows++] = t - 1;
    } else {
      if (in.sample_last[s] && cnt > 0) rows[n_rows++] = t - 1;
      ++p_row;
    }
  }
  return STEP_PACK_OK;
}

}  // namespace ps
