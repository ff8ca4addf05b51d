// A program of its own around csrc/boot_host.cpp, built under the host sanitizers by tests/test_boot_host.py.  Reads commands, one
// per line, from the file named on the command line and prints one line per command:
//   draws SEED REP NCOLS              -> "draws c_0 c_1 ..."            (pml_boot_draws_host)
//   counts SEED REP NPAT L p_0 ..     -> "counts n_0 .. | idx i_0 .."   (boot_counts_host, boot_compact_host)
//   total N ns_0 ..                   -> "total L" or "total error MESSAGE"
//   pseed SEED WHICH                  -> "pseed S"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../include/peprml.h"
#include "../../pepr_amd/csrc/boot.hpp"

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string cmd; ss >> cmd;
        if (cmd == "draws") {
            unsigned long long seed; int rep; long long n; ss >> seed >> rep >> n;
            std::vector<unsigned> cols((size_t)(n > 0 && n < (1ll << 31) ? n : 1));
            const int rc = pml_boot_draws_host(seed, rep, n, cols.data());
            if (rc) { std::cout << "draws error " << rc << "\n"; continue; }
            std::cout << "draws";
            for (long long j = 0; j < n; ++j) std::cout << ' ' << cols[(size_t)j];
            std::cout << "\n";
        } else if (cmd == "counts") {
            unsigned long long seed; int rep, npat; size_t L; ss >> seed >> rep >> npat >> L;
            std::vector<int> c2p(L); for (auto &v : c2p) ss >> v;
            std::vector<uint32_t> count; std::vector<int> idx;
            pml::boot_counts_host(seed, rep, c2p, npat, count);
            pml::boot_compact_host(count, idx);
            std::cout << "counts";
            for (auto v : count) std::cout << ' ' << v;
            std::cout << " | idx";
            for (auto v : idx) std::cout << ' ' << v;
            std::cout << "\n";
        } else if (cmd == "total") {
            int n; ss >> n;
            std::vector<long long> ns((size_t)n); for (auto &v : ns) ss >> v;
            std::string err;
            const long long L = pml::boot_total_columns(n, ns.data(), err);
            if (L < 0) std::cout << "total error " << err << "\n"; else std::cout << "total " << L << "\n";
        } else if (cmd == "pseed") {
            unsigned long long seed; int which; ss >> seed >> which;
            std::cout << "pseed " << pml::boot_parsimony_seed(seed, which) << "\n";
        }
    }
    return 0;
}
