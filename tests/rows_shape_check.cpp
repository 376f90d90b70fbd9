// rows_shape_check.cpp -- the row-group launch shape (csrc/tk_rows.h) on its own: tests/test_rows_shape_cpu.py compiles this with
// -fsanitize=address,undefined and runs it.  It calls the very functions the launchers and the kernels call and checks, against
// plain divisions: units from L, rb and row_of for every units up to the tile and every unit index of a block, rows longer than
// the tile, both L == 0 behaviours and grid x.  Exit status 0 and "ok <checks>", or the first failure on stderr and 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../tekken-rs_amd/csrc/tk_rows.h"

static uint64_t n_checks = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        ++n_checks;                                                        \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);     \
            fprintf(stderr, __VA_ARGS__);                                  \
            fprintf(stderr, "\n");                                         \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static const uint32_t TILE = TKY_ROWS_TILE;

static uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
static uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// an L < 2^31 that has `units` units a row: units itself, element by element, or 4 * units where units is a multiple of 4
static uint32_t len_of(uint32_t units) { return units % 4u ? units : 4u * units; }

// the shape of L: the same for every n_rows > 0, and grid x over the row counts around rb
static TkyRows shape_of(uint32_t L, bool unit_of_empty_row) {
    TkyRows want = {0u, 0u, 0u};
    tky_rows_shape(1, L, unit_of_empty_row, want);
    const uint64_t ns[] = {0, 1, want.rb, (uint64_t)want.rb + 1u, 0xFFFFFFFFull};
    for (uint64_t n : ns) {
        TkyRows s = {0u, 0u, 0u};
        const TkyRowsGrid g = tky_rows_shape(n, L, unit_of_empty_row, s);
        CHECK(g.x == min64(ceil_div(n, want.rb), 1u << 20), "L %u n_rows %llu: grid x %u", L, (unsigned long long)n, g.x);
        if (n == 0) continue;
        CHECK(s.units == want.units && s.rb == want.rb && s.magic == want.magic, "L %u n_rows %llu: another shape", L, (unsigned long long)n);
        CHECK(tky_row_groups(s, n) == ceil_div(n, want.rb), "L %u n_rows %llu: row groups", L, (unsigned long long)n);
        CHECK(g.y == (want.rb == 1u ? min64(ceil_div(want.units, TILE), 64u) : 1u), "L %u n_rows %llu: grid y %u", L, (unsigned long long)n, g.y);
    }
    return want;
}

int main() {
    // units from L: groups of 4 elements where L % 4 == 0, single elements otherwise
    for (uint32_t L = 1; L <= 4u * TILE + 8u; ++L) {
        TkyRows s = {0u, 0u, 0u};
        tky_rows_shape(1, L, false, s);
        CHECK(s.units == (L % 4u == 0u ? L / 4u : L), "L %u: units %u", L, s.units);
    }
    // every units up to the tile: the rows of a block fill the tile and no more, and the reciprocal is the division
    for (uint32_t units = 1; units <= TILE; ++units) {
        const TkyRows s = shape_of(len_of(units), false);
        CHECK(s.units == units, "units %u: got %u", units, s.units);
        CHECK(s.rb == TILE / units && (uint64_t)s.rb * units <= TILE, "units %u: rb %u", units, s.rb);
        for (uint32_t li = 0; li < s.rb * units; ++li)
            CHECK(tky_row_of(s, li) == li / units, "units %u: row_of(%u) = %u", units, li, tky_row_of(s, li));
    }
    // rows longer than the tile: one block row, split over y
    const uint32_t big[] = {TILE + 1u, 2u * TILE, 64u * TILE, 64u * TILE + 1u, 0x7FFFFFFFu};
    for (uint32_t units : big) {
        const TkyRows s = shape_of(len_of(units), false);
        CHECK(s.units == units && s.rb == 1u, "units %u: units %u rb %u", units, s.units, s.rb);
        TkyRows s3 = {0u, 0u, 0u};
        const TkyRowsGrid g = tky_rows_shape(3, len_of(units), true, s3);
        CHECK(g.x == 3u && g.y == min64(ceil_div(units, TILE), 64u), "units %u: grid %u x %u", units, g.x, g.y);
        const uint32_t lis[] = {0u, 1u, TILE, units - 1u};
        for (uint32_t li : lis) CHECK(tky_row_of(s, li) == 0u, "units %u: row_of(%u) = %u", units, li, tky_row_of(s, li));
    }
    // L == 0: nothing to launch, or one unit a row; no rows: nothing to launch
    TkyRows s = {0u, 0u, 0u};
    CHECK(tky_rows_shape(5, 0, false, s).x == 0u, "L 0, no unit: something to launch");
    s = shape_of(0, true);
    CHECK(s.units == 1u && s.rb == TILE, "L 0, one unit a row: units %u rb %u", s.units, s.rb);
    for (uint32_t li = 0; li < TILE; ++li) CHECK(tky_row_of(s, li) == li, "L 0: row_of(%u)", li);
    CHECK(tky_rows_shape(0, 0, true, s).x == 0u && tky_rows_shape(0, 8, true, s).x == 0u && tky_rows_shape(0, 8, false, s).x == 0u, "no rows: something to launch");
    printf("ok %llu\n", (unsigned long long)n_checks);
    return 0;
}
