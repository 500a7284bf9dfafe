// openmavis_amd/csrc/omv_topk.h on the host (tests/test_topk_insert_cpu.py).  One sequence of keys per input line
// (decimal, blank-separated): they are inserted one by one into an empty 16-slot list, and the list after every insert
// is printed as one line of 16 hexadecimal words.  A line `end` follows each sequence.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../openmavis_amd/csrc/omv_topk.h"

constexpr int kTop = 16;

int main() {
    std::string line;
    for (int c; (c = getchar()) != EOF;) {
        if (c != '\n') {
            line.push_back((char)c);
            continue;
        }
        std::vector<uint32_t> key(kTop, ~0u);   // on the heap: an access past the list is the sanitizer's to report
        const char *p = line.c_str();
        for (char *e;; p = e) {
            const unsigned long long v = strtoull(p, &e, 10);
            if (e == p) break;
            omv::topk_insert<kTop>(key.data(), (uint32_t)v);
            for (int q = 0; q < kTop; ++q) printf("%08" PRIx32 "%c", key[q], q + 1 < kTop ? ' ' : '\n');
        }
        puts("end");
        line.clear();
    }
    return 0;
}
