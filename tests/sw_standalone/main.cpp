// The driver of sw_host.cpp built ALONE (with nj.cpp for the table) under host sanitizers (tests/test_sw_host.py): reads a proteome
// set from stdin -- a line `G` opens a genome, `P <label> [<residues>]` adds a protein -- and prints pml_sw_search_host's return
// code and table.  argv[1] = traceback (0 / 1), argv[2] = the E-value cutoff.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/peprml.h"

int main(int argc, char **argv) {
    std::vector<std::string> labels, residues;
    std::vector<int> off(1, 0);
    std::string line;
    bool open = false;
    while (std::getline(std::cin, line)) {
        if (line == "G") { if (open) off.push_back((int)labels.size()); open = true; continue; }
        if (line.rfind("P ", 0) != 0) continue;
        std::istringstream in(line.substr(2));
        std::string lab, res;
        in >> lab >> res;
        labels.push_back(lab); residues.push_back(res);
    }
    if (open) off.push_back((int)labels.size());
    std::vector<const char *> lp, rp;
    for (auto &s : labels) lp.push_back(s.c_str());
    for (auto &s : residues) rp.push_back(s.c_str());
    pml_proteome_set set;
    set.ngenomes = (int)off.size() - 1; set.genome_off = off.data(); set.labels = lp.data(); set.residues = rp.data();
    pml_sw_opts o;
    std::memset(&o, 0, sizeof o);
    o.traceback = argc > 1 ? std::atoi(argv[1]) : 0;
    o.evalue = argc > 2 ? std::atof(argv[2]) : 0.0;
    pml_sw_result r;
    const int rc = pml_sw_search_host(&set, &o, &r);
    std::printf("rc %d hits %lld cells %lld\n", rc, rc ? 0LL : r.nhits, rc ? 0LL : r.cells);
    if (!rc) std::fwrite(r.table, 1, (size_t)r.table_bytes, stdout);
    pml_sw_result_free(&r);
    int limits[8];
    return pml_sw_class_limits(limits);
}
