// The length stamp of host.hpp's Tree under AddressSanitizer + UBSan (host code only): every writer of Tree::len renews the
// stamp, a copy carries it, and equal stamps mean equal lengths -- what Batch::replay_plan relies on when it compares stamps
// instead of bytes.  Writers driven here: parse, NJ, put_len, set_len, map_len, reset_len, assignment from a backup, on
// several threads at once (the groups of a search call build and change trees side by side).
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../pepr_amd/csrc/host.hpp"

using namespace pml;

static std::atomic<int> checks{0};
#define CHECK(c) do { ++checks; if (!(c)) { std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static bool same_lengths(const Tree &a, const Tree &b) {
    const auto &x = a.len.values(), &y = b.len.values();
    return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof x[0]) == 0);
}

// random writes, backups and undos on one tree; every state is recorded as stamp -> lengths, and a stamp seen twice must show
// the lengths it showed first
static int churn(unsigned seed, const Tree &start, std::vector<unsigned long long> &stamps_out) {
    std::mt19937 rng(seed);
    Tree t = start;
    std::vector<Tree> backups{start};
    std::map<unsigned long long, std::vector<std::array<double, 3>>> seen;
    auto record = [&](const Tree &x) {
        auto it = seen.find(x.len_stamp);
        if (it == seen.end()) { seen[x.len_stamp] = x.len.values(); return true; }
        return it->second.size() == x.len.size() && std::memcmp(it->second.data(), x.len.values().data(), it->second.size() * sizeof it->second[0]) == 0;
    };
    CHECK(record(t));
    for (int it = 0; it < 4000; ++it) {
        const unsigned long long before = t.len_stamp;
        const Tree was = t;
        const int op = (int)(rng() % 6);
        if (op == 0) { const int v = (int)(rng() % (unsigned)t.nnodes()); t.put_len(v, 0, 0.001 * (double)(1 + rng() % 1000)); }
        else if (op == 1) {
            const int u = t.ntax + (int)(rng() % (unsigned)(t.nnodes() - t.ntax)), k = (int)(rng() % 3);
            t.set_len(u, t.nbr[u][k], 0.002 * (double)(1 + rng() % 1000));
        }
        else if (op == 2) t.map_len([](double x) { return x < 0.5 ? x * 1.25 : x; });
        else if (op == 3) backups.push_back(t);
        else if (op == 4) t = backups[rng() % backups.size()];          // undo / tree replacement
        else { Tree fresh = start; fresh.reset_len((size_t)start.nnodes()); CHECK(fresh.len_stamp != start.len_stamp && fresh.len.size() == start.len.size()); }
        if (op <= 2) CHECK(t.len_stamp != before && t.len_stamp != 0);          // a writer always renews, even when the value written is the old one
        if (t.len_stamp == before) CHECK(same_lengths(t, was));
        CHECK(record(t));
    }
    for (auto &kv : seen) stamps_out.push_back(kv.first);
    return 0;
}

int main() {
    std::string err;
    std::vector<std::string> names = {"a", "b", "c", "d", "e", "f"};
    Tree p, q;
    CHECK(Tree::parse("((a:0.1,b:0.2):0.05,c:0.3,((d:0.1,e:0.1):0.2,f:0.4):0.1);", names, p, err));
    CHECK(Tree::parse("((a:0.1,b:0.2):0.05,c:0.3,((d:0.1,e:0.1):0.2,f:0.5):0.1);", names, q, err));
    CHECK(p.len_stamp != 0 && q.len_stamp != 0 && p.len_stamp != q.len_stamp && !same_lengths(p, q));
    Tree none; CHECK(none.len_stamp == 0 && none.len.size() == 0);
    {   // a copy keeps the stamp, a write to the copy leaves the original's alone
        Tree c = p; CHECK(c.len_stamp == p.len_stamp && same_lengths(c, p));
        const unsigned long long s = p.len_stamp;
        c.set_len(0, c.nbr[0][0], 0.7); CHECK(c.len_stamp != s && p.len_stamp == s && !same_lengths(c, p));
        c = p; CHECK(c.len_stamp == s && same_lengths(c, p));
    }
    {   // NJ start trees: each its own stamp
        const char *nm[] = {"t0", "t1", "t2", "t3", "t4"};
        const char *rows[] = {"ARNDCQEGHI", "ARNDCQEGHL", "ARNECQEGHL", "TRNECQKGHL", "TRNECQKGHV"};
        EncodedAlignment e; CHECK(e.encode(5, 10, nm, rows, err));
        Tree a = nj_tree(e), b = nj_tree(e);
        CHECK(a.len_stamp != 0 && a.len_stamp != b.len_stamp && same_lengths(a, b));
    }
    // the clock is shared: threads that write at the same time never draw the same stamp for different lengths
    const int T = 4;
    std::vector<std::vector<unsigned long long>> stamps(T);
    std::vector<int> rcs(T, 0);
    std::vector<std::thread> th;
    for (int k = 0; k < T; ++k) th.emplace_back([&, k] { rcs[k] = churn(100u + (unsigned)k, k % 2 ? p : q, stamps[k]); });
    for (auto &t : th) t.join();
    for (int k = 0; k < T; ++k) CHECK(rcs[k] == 0);
    std::map<unsigned long long, int> owner;
    for (int k = 0; k < T; ++k) for (unsigned long long s : stamps[k]) {
        if (s == p.len_stamp || s == q.len_stamp) continue;           // the two start trees are shared on purpose
        CHECK(owner.emplace(s, k).second);
    }
    std::printf("length stamp driver: %d checks ok\n", checks.load());
    return 0;
}
