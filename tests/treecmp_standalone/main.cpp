// Stand-alone driver of pepr_amd/csrc/treecmp.cpp (with host.cpp's Newick reader) for tests/test_treecmp_host.py, which builds
// the three files with g++ -fsanitize=address,undefined and runs the program: nothing is loaded into Python.
// usage: treecmp_standalone FILE USE_LENGTHS -- FILE holds one Newick tree per line.  Prints
//   n <taxa> words <W>                     then per tree      tree <t> nreal <k> nrec <m> max <hexfloat>
//   and per record                         <flags> <length hexfloat> <length/max hexfloat> <word W-1 .. word 0 as 16 hex digits each>
// or, when the set is refused,             refused <code> <message>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/peprml.h"
#include "../../pepr_amd/csrc/treecmp.hpp"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1]);
    std::vector<std::string> lines; std::string line;
    while (std::getline(in, line)) if (!line.empty()) lines.push_back(line);
    std::vector<const char *> ptr;
    for (auto &s : lines) ptr.push_back(s.c_str());
    pml::TcSet S; std::string err;
    const int rc = pml::tc_build((int)ptr.size(), ptr.data(), std::atoi(argv[2]), S, err);
    if (rc != PML_OK) { std::printf("refused %d %s\n", rc, err.c_str()); return 0; }
    std::printf("n %d words %d\n", S.n, S.W);
    for (size_t t = 0; t < S.trees.size(); ++t) {
        const pml::TcTree &T = S.trees[t];
        std::printf("tree %zu nreal %d nrec %d max %a\n", t, T.nreal, T.nrec(), T.maxlen);
        for (int r = 0; r < T.nrec(); ++r) {
            std::printf("%d %a %a ", T.flags[(size_t)r], T.len[(size_t)r], T.lnorm[(size_t)r]);
            for (int w = S.W - 1; w >= 0; --w) std::printf("%016llx", T.words[(size_t)r * S.W + w]);
            std::printf("\n");
        }
    }
    return 0;
}
