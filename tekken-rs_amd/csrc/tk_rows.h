// tk_rows.h -- the row-group launch shape of the layout kernels that write a [n_rows, L] tensor row by row (tk_dense.hip both
// directions, tk_window.hip, tk_pair.hip).  Plain C++ without HIP, so that tests/rows_shape_check.cpp runs the very functions the
// launchers and the kernels call.
//
// The unit of work is a group of 4 consecutive elements of one row where L % 4 == 0 (one 16-byte store for int32, two for int64,
// one dword of a uint8 plane), a single element otherwise.  A block takes `rb` consecutive rows (rb * units <= TKY_ROWS_TILE,
// `units` units a row) and its threads walk the rb * units units in order, so a wave covers several short rows and every lane has
// work; the row of a unit comes from a per-launch reciprocal, not from a division.  A row of more than TKY_ROWS_TILE units is one
// block row (rb == 1) split over blockIdx.y.  The blocks stride over the row groups with gridDim.x (tk_layout.h TkyRowGroup).
#ifndef TK_ROWS_H
#define TK_ROWS_H
#include <stdint.h>

#ifdef __HIPCC__
#define TKY_HD __host__ __device__
#else
#define TKY_HD
#endif

#define TKY_ROWS_TILE 2048u    /* units of a block's row group (8 a thread); the reciprocal is exact for indices below it */

struct TkyRows { uint32_t units, rb, magic; };   // units a row, rows a block, 2^32 / units rounded up
struct TkyRowsGrid { uint32_t x, y; };           // x == 0: nothing to launch

// row groups of n_rows rows
TKY_HD inline uint64_t tky_row_groups(const TkyRows& s, uint64_t n_rows) { return (n_rows + s.rb - 1) / s.rb; }

// row of unit li inside the block's row group (li < rb * units <= TKY_ROWS_TILE when rb > 1)
TKY_HD inline uint32_t tky_row_of(const TkyRows& s, uint32_t li) {
    if (s.rb == 1u) return 0u;
    return s.units == 1u ? li : (uint32_t)(((uint64_t)li * s.magic) >> 32);
}

// The shape and the grid of a [n_rows, row_len] tensor.  row_len == 0: nothing to launch, or -- unit_of_empty_row -- one unit a
// row, for the kernels whose first unit of a row writes the per-row outputs.
inline TkyRowsGrid tky_rows_shape(uint64_t n_rows, uint32_t row_len, bool unit_of_empty_row, TkyRows& s) {
    s.units = row_len == 0u ? (unit_of_empty_row ? 1u : 0u) : row_len % 4u == 0u ? row_len / 4u : row_len;
    if (n_rows == 0 || s.units == 0u) return TkyRowsGrid{0u, 0u};
    s.rb = s.units <= TKY_ROWS_TILE ? TKY_ROWS_TILE / s.units : 1u;
    s.magic = s.units > 1u ? (uint32_t)((1ull << 32) / s.units) + 1u : 0u;
    const uint64_t gx = tky_row_groups(s, n_rows), gy = s.rb == 1u ? (s.units + TKY_ROWS_TILE - 1) / TKY_ROWS_TILE : 1u;
    return TkyRowsGrid{(uint32_t)(gx < (1u << 20) ? gx : 1u << 20), (uint32_t)(gy < 64u ? gy : 64u)};
}

#endif
