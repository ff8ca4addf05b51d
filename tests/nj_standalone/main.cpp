// Stand-alone driver of pepr_amd/csrc/nj.cpp for the host sanitizers (tests/test_nj_host.py builds both files with
// g++ -fsanitize=address,undefined and runs the program: nothing is loaded into Python).  Seeded random matrices, n = 4..40,
// integer-valued with many ties and arbitrary doubles, both matrix types and both forms, through the C entry points; the
// encoder on every byte value; the program prints a checksum of the texts so that two builds can be compared.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/peprml.h"
#include "../../pepr_amd/csrc/nj.hpp"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t next() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }

int main() {
    uint64_t sum = 1469598103934665603ull; long trees = 0;
    for (int round = 0; round < 120; ++round) {
        const int n = 4 + (int)(next() % 37);
        std::vector<std::string> names; std::vector<const char *> ptr;
        for (int i = 0; i < n; ++i) names.push_back("t" + std::to_string(i));
        for (auto &s : names) ptr.push_back(s.c_str());
        std::vector<double> m((size_t)n * n);
        const int kind = round % 3;
        for (int i = 0; i < n; ++i)
            for (int j = i; j < n; ++j) {
                double v = kind == 0 ? (double)(next() % 4) : kind == 1 ? (double)(int64_t)(next() % 2001) - 1000.0 : (double)(next() >> 11) / 9007199254740992.0 * 50.0;
                m[(size_t)i * n + j] = v; m[(size_t)j * n + i] = (round & 8) ? v + (double)(next() % 2) : v;       // some asymmetric
            }
        for (int type = 0; type < 2; ++type)
            for (int form = 0; form < 2; ++form) {
                char *out = nullptr;
                const int rc = pml_nj_from_matrix(n, ptr.data(), m.data(), type, form, &out);
                if (rc != PML_OK || !out) { std::fprintf(stderr, "round %d type %d form %d: rc %d\n", round, type, form, rc); return 1; }
                for (const char *p = out; *p; ++p) sum = (sum ^ (unsigned char)*p) * 1099511628211ull;
                std::free(out); ++trees;
            }
    }
    char *out = nullptr;
    double three[9] = {0, 1, 2, 1, 0, 3, 2, 3, 0}; const char *nm[3] = {"a", "b", "c"};
    if (pml_nj_from_matrix(3, nm, three, 0, 0, &out) != PML_EINVAL || out) return 2;
    if (pml_nj_from_matrix(4, nullptr, three, 0, 0, &out) != PML_EINVAL) return 3;
    int table[576];
    if (pml_pairscore_table_blosum62(table) != PML_OK || table[21 * 24 + 21] != 3 || table[23 * 24 + 5] != 0) return 4;
    char row[256]; uint8_t codes[256]; int bad = 0;
    for (int b = 1; b < 256; ++b) {
        std::memset(row, 'A', sizeof row); row[b] = (char)b;
        int col = -1, byte = -1;
        if (pml::nj_encode24(row, 256, codes, &col, &byte)) { if (col != b || byte != b) return 5; ++bad; }
    }
    std::printf("nj_standalone ok: %ld trees, %d refused bytes, checksum %016llx\n", trees, bad, (unsigned long long)sum);
    return bad == 255 - (2 * 23 + 2) ? 0 : 6;
}
