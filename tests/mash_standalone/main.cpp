// A small program around pepr_amd/csrc/mash_host.cpp alone (no HIP, no library), built by tests/test_mash_host.py with
// -fsanitize=address,undefined and run as a process of its own.  It reads commands from a file and prints what the host rule gives:
//   G k s nrec            then nrec lines, a record's bytes in hex ("-" = an empty record): "values ...", "sketch ..."
//   P k s na nb           then a line of na and a line of nb values ("-" = none): "pair common denom distance"
//   T n                   then n distances: "stats mean sd max"
//   E n_in n_pool target  then n_pool rows of n_in distances and a line of n_pool flags: "expand ..."
//   S n count max sd      then n distances: "select ..."
// Doubles are printed as hexadecimal floats.  A refused input prints "error <code>".
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/peprml.h"

static std::string unhex(const std::string &h) {
    std::string out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return out;
}

static std::vector<unsigned long long> numbers(const std::string &line) {
    std::vector<unsigned long long> v;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok) if (tok != "-") v.push_back(std::stoull(tok));
    return v;
}

static std::vector<double> doubles(const std::string &line) {
    std::vector<double> v;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok) v.push_back(std::stod(tok));
    return v;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        char cmd = 0;
        in >> cmd;
        if (cmd == 'G') {
            int k, s, nrec;
            in >> k >> s >> nrec;
            std::vector<std::string> recs;
            for (int r = 0; r < nrec; ++r) { std::getline(f, line); recs.push_back(unhex(line)); }
            std::vector<const char *> ptr;
            std::vector<long long> len;
            size_t total = 0;
            for (auto &r : recs) { ptr.push_back(r.data()); len.push_back((long long)r.size()); total += r.size(); }
            pml_genome g{nrec, ptr.data(), len.data()};
            std::vector<unsigned long long> v(total + 1), sk((size_t)(s > 0 ? s : 1));
            int n = 0, rc = pml_mash_hashes_host(&g, k, v.data());
            if (!rc) rc = pml_mash_sketch_host(&g, k, s, sk.data(), &n);
            if (rc) { std::printf("error %d\n", rc); continue; }
            std::printf("values");
            for (size_t i = 0; i < total; ++i) std::printf(" %llx", v[i]);
            std::printf("\nsketch");
            for (int i = 0; i < n; ++i) std::printf(" %llx", sk[(size_t)i]);
            std::printf("\n");
        } else if (cmd == 'P') {
            int k, s, na, nb;
            in >> k >> s >> na >> nb;
            std::getline(f, line); std::vector<unsigned long long> a = numbers(line);
            std::getline(f, line); std::vector<unsigned long long> b = numbers(line);
            int c = 0, d = 0;
            const int rc = pml_mash_pair_host(a.data(), (int)a.size(), b.data(), (int)b.size(), s, &c, &d);
            if (rc) { std::printf("error %d\n", rc); continue; }
            std::printf("pair %d %d %a %a\n", c, d, pml_mash_distance_of(c, d, k, 0), pml_mash_distance_of(c, d, k, 6));
        } else if (cmd == 'T') {
            int n;
            in >> n;
            std::getline(f, line); std::vector<double> d = doubles(line);
            double out[3];
            const int rc = pml_mash_pair_stats((int)d.size(), d.data(), out);
            if (rc) { std::printf("error %d\n", rc); continue; }
            std::printf("stats %a %a %a\n", out[0], out[1], out[2]);
        } else if (cmd == 'E') {
            int n_in, n_pool, target;
            in >> n_in >> n_pool >> target;
            std::vector<double> d;
            for (int p = 0; p < n_pool; ++p) { std::getline(f, line); for (double x : doubles(line)) d.push_back(x); }
            std::getline(f, line); std::vector<unsigned long long> fl = numbers(line);
            std::vector<unsigned char> flags(fl.begin(), fl.end());
            flags.resize((size_t)n_pool + 1, 0);
            std::vector<int> added((size_t)n_pool + 1);
            std::vector<double> cand((size_t)n_pool + 1);
            int na = 0, rc = (int)d.size() == n_in * n_pool ? pml_mash_expand_ingroup(n_in, n_pool, d.data(), flags.data(), target, added.data(), &na) : PML_EINVAL;
            if (!rc) rc = pml_mash_candidate_distances(n_in, n_pool, d.data(), cand.data());
            if (rc) { std::printf("error %d\n", rc); continue; }
            std::printf("expand");
            for (int i = 0; i < na; ++i) std::printf(" %d", added[(size_t)i]);
            std::printf("\ncandidates");
            for (int p = 0; p < n_pool; ++p) std::printf(" %a", cand[(size_t)p]);
            std::printf("\n");
        } else if (cmd == 'S') {
            int n, count;
            std::string mx, sd;
            in >> n >> count >> mx >> sd;
            std::getline(f, line); std::vector<double> c = doubles(line);
            std::vector<int> sel(c.size() + 1);
            int ns = 0;
            const int rc = pml_mash_select_outgroup((int)c.size(), c.data(), std::stod(mx), std::stod(sd), count, sel.data(), &ns);
            if (rc) { std::printf("error %d\n", rc); continue; }
            std::printf("select");
            for (int i = 0; i < ns; ++i) std::printf(" %d", sel[(size_t)i]);
            std::printf("\n");
        }
    }
    return 0;
}
