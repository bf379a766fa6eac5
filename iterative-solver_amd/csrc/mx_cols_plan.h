// Column plan of ssp_q32_gemm_inner_cols (kernels_mixed.hip): an inner product whose column list mixes
// f64 and f32 vectors in any order.  No HIP here: tests/test_q32_fused_boundary.py drives it on the CPU.
//
// The kernel's unit is a group of 4 columns with one storage type.  The plan lays the caller's k columns
// out in `slots` column slots: the f64 columns first, in the caller's order, padded to whole groups of 4,
// then the f32 columns likewise.  A padding slot holds no column (slot_col = -1); only the last group of
// a type's run has any, so the first slot of every group is a column.  The slots are cut into tiles of at
// most max_rows x max_cols (max_cols a multiple of 4), each with its f64 groups leading (g64 of them).
// The m x slots result is what is summed over ranks: its layout depends on (m, k, the types) only.
#pragma once
#include <algorithm>
#include <vector>

namespace ssp {

struct ColsTile {
  int r0, rows;  // rows [r0, r0 + rows)
  int c0, cols;  // slots [c0, c0 + cols), cols a multiple of 4
  int g64;       // the tile's first g64 groups are f64, the others f32
};

struct ColsPlan {
  int m = 0, k = 0;
  int n64 = 0, n32 = 0;       // columns of each type
  int slots = 0;              // 4 ceil(n64 / 4) + 4 ceil(n32 / 4)
  std::vector<int> slot_col;  // [slots] the caller's column in the slot, -1: padding
  std::vector<int> col_slot;  // [k] the slot of the caller's column (the permutation back)
  std::vector<ColsTile> tiles;
};

// f32[j] != 0: column j is stored in f32.
inline ColsPlan plan_cols(int m, const unsigned char* f32, int k, int max_rows, int max_cols) {
  ColsPlan p;
  p.m = m;
  p.k = k;
  for (int j = 0; j < k; ++j) (f32[j] ? p.n32 : p.n64)++;
  const int s64 = 4 * ((p.n64 + 3) / 4), s32 = 4 * ((p.n32 + 3) / 4);
  p.slots = s64 + s32;
  p.slot_col.assign(size_t(p.slots), -1);
  p.col_slot.assign(size_t(k), -1);
  int next64 = 0, next32 = s64;
  for (int j = 0; j < k; ++j) {
    const int s = f32[j] ? next32++ : next64++;
    p.slot_col[size_t(s)] = j;
    p.col_slot[size_t(j)] = s;
  }
  for (int r0 = 0; r0 < m; r0 += max_rows)
    for (int c0 = 0; c0 < p.slots; c0 += max_cols) {
      ColsTile t;
      t.r0 = r0;
      t.rows = std::min(max_rows, m - r0);
      t.c0 = c0;
      t.cols = std::min(max_cols, p.slots - c0);
      t.g64 = std::max(0, std::min(s64 - c0, t.cols)) / 4;
      p.tiles.push_back(t);
    }
  return p;
}

}  // namespace ssp
