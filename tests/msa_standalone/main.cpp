// The driver of msa_host.cpp built ALONE (with sw_host.cpp, and nj.cpp for the table) under host sanitizers
// (tests/test_msa_host.py): reads sets from stdin -- a line `S` opens a set, `Q <residues>` adds a sequence -- and prints
// pml_msa_align_host's return code, then per set its aligned rows and its merges.  argv[1] / argv[2] = gap_open / gap_extend.
// A line `P` instead of `S` opens a profile: the first two profiles are aligned with pml_msa_profile_align_host as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/peprml.h"

int main(int argc, char **argv) {
    std::vector<std::vector<std::string>> sets, profiles;
    std::string line;
    std::vector<std::vector<std::string>> *into = nullptr;
    while (std::getline(std::cin, line)) {
        if (line == "S") { sets.emplace_back(); into = &sets; continue; }
        if (line == "P") { profiles.emplace_back(); into = &profiles; continue; }
        if (line.rfind("Q ", 0) == 0 && into) into->back().push_back(line.substr(2));
        else if (line == "Q" && into) into->back().push_back("");
    }
    pml_msa_opts o;
    std::memset(&o, 0, sizeof o);
    o.gap_open = argc > 1 ? std::atoi(argv[1]) : 0;
    o.gap_extend = argc > 2 ? std::atoi(argv[2]) : 0;
    auto as_sets = [](const std::vector<std::vector<std::string>> &v, std::vector<std::vector<const char *>> &ptrs) {
        std::vector<pml_msa_set> out;
        ptrs.resize(v.size());
        for (size_t s = 0; s < v.size(); ++s) {
            for (auto &q : v[s]) ptrs[s].push_back(q.c_str());
            pml_msa_set st; st.nseq = (int)v[s].size(); st.residues = ptrs[s].data();
            out.push_back(st);
        }
        return out;
    };
    auto print = [](const pml_msa_result &r) {
        for (int i = 0; i < r.nrows; ++i) std::printf("row %s\n", r.rows + (size_t)i * ((size_t)r.ncols + 1));
        for (int m = 0; m < r.nmerges; ++m) std::printf("merge %d %d %d %lld\n", r.merge_x[m], r.merge_y[m], r.merge_level[m], r.merge_score[m]);
    };
    char err[256] = "";
    std::vector<std::vector<const char *>> p1, p2;
    std::vector<pml_msa_set> ss = as_sets(sets, p1), pp = as_sets(profiles, p2);
    std::vector<pml_msa_result> res(ss.size() + 1);
    const int rc = pml_msa_align_host((int)ss.size(), ss.data(), &o, res.data(), err, (int)sizeof err);
    std::printf("rc %d %s\n", rc, err);
    for (size_t s = 0; s < ss.size() && !rc; ++s) { std::printf("set %zu\n", s); print(res[s]); pml_msa_result_free(&res[s]); }
    if (pp.size() >= 2) {
        pml_msa_result r; long long score = 0;
        const int rc2 = pml_msa_profile_align_host(&pp[0], &pp[1], &o, &score, &r, err, (int)sizeof err);
        std::printf("profile rc %d score %lld\n", rc2, rc2 ? 0LL : score);
        if (!rc2) { print(r); std::printf("path "); for (int c = 0; c < r.ncols; ++c) std::printf("%d", (int)r.path[c]); std::printf("\n"); }
        pml_msa_result_free(&r);
    }
    int limits[8];
    return pml_msa_limits(limits);
}
