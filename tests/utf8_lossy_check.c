// Drives csrc/tk_utf8_lossy.h over the cases of a file (tests/test_decode_lossy_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it as a program of its own).
//
//   utf8_lossy_check CASES OUT
//
// A line of CASES: the bytes of a document in hex ("-" for none), a blank, the run starts as a hex bit mask (bit p: a run starts at
// byte p; byte 0 always starts one).  The line of OUT for it, four fields separated by blanks, "-" for nothing:
//   1. the lossy text by tkul_class, position by position (the way the repair kernels run it)
//   2. the same with the positions of TKUL_HOLD at the end of the text left out (a stream step that is not final)
//   3. the text by tkul_feed / tkul_flush at every run start, without a flush at the end (the way the stream kernels run it)
//   4. the state word tkul_feed leaves, 8 hex digits
// The bytes around the document in the buffer are FF on one side and C3 on the other: they must never matter.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../tekken-rs_amd/csrc/tk_utf8_lossy.h"

#define MAXN 64

static void put_hex(FILE* f, const uint8_t* b, size_t n) {
    if (!n) fputc('-', f);
    for (size_t i = 0; i < n; ++i) fprintf(f, "%02x", b[i]);
}

static size_t emit(uint8_t* dst, size_t at, uint32_t r, const uint8_t* tmp) {
    memcpy(dst + at, tmp, r & 0xFFu);
    return at + (r & 0xFFu);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "r");
    FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    char hex[4 * MAXN];
    unsigned long long starts;
    while (fscanf(in, "%255s %llx", hex, &starts) == 2) {
        uint8_t buf[MAXN + 8];
        memset(buf, 0xFF, 4);
        size_t n = 0;
        if (hex[0] != '-') {
            n = strlen(hex) / 2;
            if (n > MAXN - 8) return 3;
            for (size_t i = 0; i < n; ++i) {
                unsigned v;
                sscanf(hex + 2 * i, "%2x", &v);
                buf[4 + i] = (uint8_t)v;
            }
        }
        memset(buf + 4 + n, 0xC3, 4);
        const uint8_t* doc = buf + 4;
        starts |= 1ull;
        uint8_t full[3 * MAXN], held[3 * MAXN], fed[3 * MAXN], tmp[8];
        size_t nf = 0, nh = 0, nd = 0;
        for (size_t p = 0; p < n; ++p) {
            uint32_t nb = 0, na = 0;
            while (nb < 3 && !((starts >> (p - nb)) & 1ull)) ++nb;          // (bit 0 is set: p - nb never goes below 0)
            while (na < 3 && p + na + 1 < n && !((starts >> (p + na + 1)) & 1ull)) ++na;
            uint64_t win = 0;
            for (int k = 0; k < 7; ++k) win |= (uint64_t)doc[(long)p - 3 + k] << (8 * k);
            const uint32_t c = tkul_class(win, nb, na);
            const uint32_t len = c & TKUL_LEN_MASK;
            // a held position: its truncated prefix ends at the end of its run, and that run is the text's last
            int at_end = (c & TKUL_HOLD) != 0;
            for (size_t q = p + 1; q < n && at_end; ++q)
                if ((starts >> q) & 1ull) at_end = 0;
            if (len == 1) {
                full[nf++] = doc[p];
                held[nh++] = doc[p];
            } else if (len == 3) {
                full[nf++] = 0xEF; full[nf++] = 0xBF; full[nf++] = 0xBD;
                if (!at_end) { held[nh++] = 0xEF; held[nh++] = 0xBF; held[nh++] = 0xBD; }
            }
        }
        uint32_t st = 0;
        for (size_t p = 0; p < n; ++p) {
            if (p && ((starts >> p) & 1ull)) nd = emit(fed, nd, tkul_flush(&st, tmp), tmp);
            nd = emit(fed, nd, tkul_feed(&st, doc[p], tmp), tmp);
        }
        put_hex(out, full, nf); fputc(' ', out);
        put_hex(out, held, nh); fputc(' ', out);
        put_hex(out, fed, nd);
        fprintf(out, " %08x\n", st);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
