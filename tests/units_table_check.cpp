// units_table_check.cpp -- the per-rank table of the units pass (csrc/tk_units_table.h) on its own: tests/test_spans_units_cpu.py
// compiles this with -fsanitize=address,undefined, feeds it tokens and compares what it prints with the definition.
// stdin: one token per line as hex digits (an empty line: the empty token).  stdout, one line per rank:
//   <entry> <n_start> <n_four> <first> <last4>        (the 16-bit entry of the table; the byte-by-byte counts of a TKU_LONG entry)
// The blob is sized exactly and the table has no slack, so a read or a write past either is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../tekken-rs_amd/csrc/tk_units_table.h"

static int hexval(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

int main() {
    std::vector<uint8_t> blob;
    std::vector<uint32_t> offs(1, 0u);
    std::string line;
    int ch;
    bool pending = false;
    while ((ch = getchar()) != EOF) {
        if (ch != '\n') { line.push_back((char)ch); pending = true; continue; }
        if (line.size() % 2) { fprintf(stderr, "odd number of hex digits\n"); return 2; }
        for (size_t k = 0; k < line.size(); k += 2) {
            const int hi = hexval(line[k]), lo = hexval(line[k + 1]);
            if (hi < 0 || lo < 0) { fprintf(stderr, "not a hex digit\n"); return 2; }
            blob.push_back((uint8_t)(hi * 16 + lo));
        }
        offs.push_back((uint32_t)blob.size());
        line.clear();
        pending = false;
    }
    if (pending) { fprintf(stderr, "the last line has no newline\n"); return 2; }
    const uint32_t n = (uint32_t)offs.size() - 1;
    // heap copies of the exact sizes: what tk_units_table_build may touch
    uint8_t* b = new uint8_t[blob.size() ? blob.size() : 1];
    if (!blob.empty()) memcpy(b, blob.data(), blob.size());
    uint16_t* tab = new uint16_t[n ? n : 1];
    tk_units_table_build(b, offs.data(), n, tab);
    for (uint32_t r = 0; r < n; ++r) {
        const TkUnitsCount c = tk_units_count(b + offs[r], offs[r + 1] - offs[r]);
        printf("%u %u %u %u %u\n", (unsigned)tab[r], c.n_start, c.n_four, c.first, c.last4);
    }
    delete[] tab;
    delete[] b;
    return 0;
}
