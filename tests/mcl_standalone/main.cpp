// Drives csrc/mcl_host.cpp alone (no HIP, no library) for a run under host sanitizers.  stdin: records
//   "G n m inflation max_iter" followed by m lines "a b w"   -> "C iters nclusters c0 c1 ..." (every node's cluster)
//   "B score_field nbytes" followed by nbytes of a hit table  -> the bidirectional filter's text, then "."
//   "F nbytes" followed by nbytes                             -> filterHitPairFile's text (or "EINVAL"), then "."
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/peprml.h"

static std::string read_bytes(long long n) {
    std::string s((size_t)n, '\0');
    if (n > 0 && std::fread(&s[0], 1, (size_t)n, stdin) != (size_t)n) std::exit(3);
    return s;
}

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'G') {
            int n, max_iter; long long m; double inflation;
            if (std::scanf("%d %lld %lf %d", &n, &m, &inflation, &max_iter) != 4) return 2;
            std::vector<int> a((size_t)m), b((size_t)m), cl((size_t)(n > 0 ? n : 1));
            std::vector<double> w((size_t)m);
            for (long long i = 0; i < m; ++i) if (std::scanf("%d %d %lf", &a[(size_t)i], &b[(size_t)i], &w[(size_t)i]) != 3) return 2;
            pml_mcl_opts o = {inflation, 0, 0, max_iter, 0};
            int nc = 0, it = 0;
            const int rc = pml_mcl_cluster_host(n, m, a.data(), b.data(), w.data(), &o, cl.data(), &nc, &it);
            if (rc) { std::printf("E %d\n", rc); continue; }
            std::printf("C %d %d", it, nc);
            for (int i = 0; i < n; ++i) std::printf(" %d", cl[(size_t)i]);
            std::printf("\n");
        } else if (kind == 'B' || kind == 'F') {
            int field = 11; long long nbytes;
            if (kind == 'B' ? std::scanf("%d %lld", &field, &nbytes) != 2 : std::scanf("%lld", &nbytes) != 1) return 2;
            std::getchar();                                            // the newline behind the header
            const std::string t = read_bytes(nbytes);
            char *out = nullptr;
            const int rc = kind == 'B' ? pml_hits_bidirectional_host(t.data(), nbytes, field, &out) : pml_hits_filter_host(t.data(), nbytes, &out);
            if (rc) std::printf("EINVAL\n.\n");
            else { std::printf("%s.\n", out); std::free(out); }
        } else return 2;
    }
    return 0;
}
