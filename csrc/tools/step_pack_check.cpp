// Stand-alone boundary check of csrc/step_pack.h, meant for a sanitizer
// build on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Icsrc csrc/tools/step_pack_check.cpp -o step_pack_check
//   ./step_pack_check
// Every case packs into an exactly-sized heap buffer (so one byte past the
// end is a sanitizer error), recomputes each section the simple way and
// compares. Exits non-zero on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "step_pack.h"

namespace {

struct Seq {
  int32_t start, count;
  bool decode, sample_last;
  int32_t prev_row;
  std::vector<int64_t> ids;
  std::vector<int32_t> table;
};

int failures = 0;

#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                    \
    }                                                                \
  } while (0)

Seq make(int32_t start, int32_t count, bool decode, bool sample_last,
         int bs, int extra_blocks = 0, int32_t prev_row = -1) {
  static int32_t next_block = 5;
  Seq s{start, count, decode, sample_last, prev_row, {}, {}};
  for (int32_t j = 0; j < count; ++j) s.ids.push_back(100 + start + j);
  const int blocks = (start + count + bs - 1) / bs + extra_blocks;
  for (int b = 0; b < blocks; ++b) {
    next_block = (next_block * 37 + 11) % 4093;
    s.table.push_back(next_block);
  }
  return s;
}

struct Flat {
  std::vector<int32_t> start, count, prev, tables;
  std::vector<uint8_t> dec, samp;
  std::vector<int64_t> ids, off;
  ps::StepPackIn in;
};

void flatten(const std::vector<Seq>& seqs, int bs, int tile, Flat* f) {
  f->off.push_back(0);
  for (const Seq& s : seqs) {
    f->start.push_back(s.start);
    f->count.push_back(s.count);
    f->prev.push_back(s.prev_row);
    f->dec.push_back(s.decode);
    f->samp.push_back(s.sample_last);
    f->ids.insert(f->ids.end(), s.ids.begin(), s.ids.end());
    f->tables.insert(f->tables.end(), s.table.begin(), s.table.end());
    f->off.push_back((int64_t)f->tables.size());
  }
  f->in.num_seqs = (int64_t)seqs.size();
  f->in.start = f->start.data();
  f->in.num_tokens = f->count.data();
  f->in.is_decode = f->dec.data();
  f->in.sample_last = f->samp.data();
  f->in.prev_row = f->prev.data();
  f->in.token_ids = f->ids.data();
  f->in.num_token_ids = (int64_t)f->ids.size();
  f->in.tables = f->tables.data();
  f->in.num_table_entries = (int64_t)f->tables.size();
  f->in.table_off = f->off.data();
  f->in.block_size = bs;
  f->in.tile_rows = tile;
}

// packs `seqs` into an exact-size buffer and checks every section
void check(const char* name, const std::vector<Seq>& seqs, int bs, int tile,
           int want_status = ps::STEP_PACK_OK) {
  std::printf("case %s\n", name);
  Flat f;
  flatten(seqs, bs, tile, &f);
  ps::StepPackLayout L;
  int st = ps::step_pack(f.in, nullptr, 0, &L);
  if (want_status != ps::STEP_PACK_OK) {
    EXPECT(st == want_status);
    // a roomy buffer must stay untouched too
    void* p = std::aligned_alloc(16, 1 << 16);
    std::memset(p, 0x5A, 1 << 16);
    EXPECT(ps::step_pack(f.in, p, 1 << 16, &L) == want_status);
    for (int i = 0; i < (1 << 16); ++i) {
      if (static_cast<unsigned char*>(p)[i] != 0x5A) {
        EXPECT(!"buffer written on a failed pack");
        break;
      }
    }
    std::free(p);
    return;
  }
  EXPECT(st == ps::STEP_PACK_TOO_SMALL);
  const int64_t need = L.total_bytes;
  EXPECT(need > 0 && need % 16 == 0);

  // one byte short: must fail and leave the buffer alone
  char* shortbuf = static_cast<char*>(std::aligned_alloc(16, (size_t)need));
  std::memset(shortbuf, 0x5A, (size_t)need);
  EXPECT(ps::step_pack(f.in, shortbuf, need - 1, &L) ==
         ps::STEP_PACK_TOO_SMALL);
  for (int64_t i = 0; i < need; ++i) {
    if (shortbuf[i] != 0x5A) {
      EXPECT(!"buffer written on a too-small pack");
      break;
    }
  }
  std::free(shortbuf);

  // exact size: anything past the end trips the sanitizer
  char* buf = static_cast<char*>(std::aligned_alloc(16, (size_t)need));
  EXPECT(ps::step_pack(f.in, buf, need, &L) == ps::STEP_PACK_OK);
  EXPECT(L.total_bytes == need);
  EXPECT(std::memcmp(buf, &L, sizeof(L)) == 0);
  auto i32 = [&](int64_t off) {
    return reinterpret_cast<const int32_t*>(buf + off);
  };
  auto i64 = [&](int64_t off) {
    return reinterpret_cast<const int64_t*>(buf + off);
  };
  int64_t max_bt = seqs.empty() ? 1 : 0;
  for (const Seq& s : seqs) {
    if ((int64_t)s.table.size() > max_bt) max_bt = (int64_t)s.table.size();
  }
  EXPECT(L.max_bt == max_bt);
  int64_t t = 0, p_row = 0, d_row = 0, tiles = 0, rows = 0, ph = 0;
  for (const Seq& s : seqs) {
    const int32_t* bt = s.decode
        ? i32(L.off_decode_block_tables) + d_row * max_bt
        : i32(L.off_prefill_block_tables) + p_row * max_bt;
    for (int64_t b = 0; b < max_bt; ++b) {
      EXPECT(bt[b] == (b < (int64_t)s.table.size() ? s.table[b] : 0));
    }
    if (!s.decode) {
      for (int32_t t0 = 0; t0 < s.count; t0 += tile) {
        const int32_t* ti = i32(L.off_prefill_tiles) + 4 * tiles++;
        EXPECT(ti[0] == p_row && ti[1] == t + t0 && ti[2] == s.start + t0);
        EXPECT(ti[3] == (s.count - t0 < tile ? s.count - t0 : tile));
      }
    }
    for (int32_t j = 0; j < s.count; ++j, ++t) {
      const int64_t pos = s.start + j;
      EXPECT(i64(L.off_tokens)[t] == s.ids[j]);
      EXPECT(i32(L.off_positions)[t] == pos);
      EXPECT(i64(L.off_slot_mapping)[t] ==
             (int64_t)s.table[pos / bs] * bs + pos % bs);
      const bool is_ph = s.decode && s.ids[j] < 0;
      EXPECT(i32(L.off_prev_row)[t] == (is_ph ? s.prev_row : -1));
      ph += is_ph;
      if (!s.decode) {
        EXPECT(i32(L.off_prefill_token_seq)[t] == p_row);
        EXPECT(i32(L.off_prefill_token_pos)[t] == pos);
      }
    }
    if (s.decode) {
      EXPECT(i32(L.off_decode_seq_lens)[d_row] == s.start + 1);
      EXPECT(i64(L.off_sample_rows)[rows++] == t - 1);
      ++d_row;
    } else {
      if (s.sample_last && s.count > 0) {
        EXPECT(i64(L.off_sample_rows)[rows++] == t - 1);
      }
      ++p_row;
    }
  }
  EXPECT(L.num_tokens == t && L.num_prefill_seqs == p_row &&
         L.num_decode_seqs == d_row && L.num_tiles == tiles &&
         L.num_sample_rows == rows && L.num_placeholders == ph);
  std::free(buf);
}

}  // namespace

int main() {
  const int bs = 16;
  for (int tile : {64, 128}) {
    check("empty", {}, bs, tile);
    check("prefill only",
          {make(0, 300, false, true, bs), make(100, 200, false, false, bs)},
          bs, tile);
    check("decode only",
          {make(5, 1, true, true, bs), make(42, 1, true, true, bs),
           make(352, 1, true, true, bs, 3)},
          bs, tile);
    check("one prefill of one row", {make(0, 1, false, true, bs)}, bs, tile);
    for (int rows : {tile - 1, tile, tile + 1, 3 * tile}) {
      check("tile edge",
            {make(7, rows, false, false, bs), make(0, rows, false, true, bs)},
            bs, tile);
    }
    for (int end : {4 * bs - 1, 4 * bs, 4 * bs + 1}) {
      check("block boundary", {make(10, end - 10, false, true, bs)}, bs, tile);
    }
    check("mixed, unequal tables",
          {make(0, 2 * tile + 3, false, true, bs),
           make(16, 34, false, false, bs, 2), make(3, 1, true, true, bs),
           make(1002, 1, true, true, bs)},
          bs, tile);
    {
      Seq a = make(13, 1, true, true, bs, 0, 6);
      a.ids[0] = -1;
      Seq b = make(31, 1, true, true, bs);
      Seq c = make(17, 1, true, true, bs, 0, 0);
      c.ids[0] = -1;
      check("decode placeholders",
            {make(0, 70, false, true, bs), a, b, c}, bs, tile);
      Seq lost = make(9, 1, true, true, bs);
      lost.ids[0] = -1;
      check("decode placeholder without a row", {lost}, bs, tile,
            ps::STEP_PACK_DECODE_UNRESOLVED);
      Seq p = make(0, 22, false, true, bs);
      p.ids[21] = -1;
      check("prefill placeholder", {p, b}, bs, tile,
            ps::STEP_PACK_PREFILL_PLACEHOLDER);
      Seq shorttab = make(0, 40, false, true, bs);
      shorttab.table.resize(1);
      check("position past the table", {shorttab}, bs, tile,
            ps::STEP_PACK_BAD_INPUT);
      check("decode before prefill", {b, make(0, 30, false, true, bs)}, bs,
            tile, ps::STEP_PACK_BAD_INPUT);
    }
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("step_pack_check: all cases passed\n");
  return 0;
}
