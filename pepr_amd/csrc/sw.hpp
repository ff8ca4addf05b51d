// sw.hpp -- what the homology search's host rule (sw_host.cpp), its device driver (sw.cpp) and its kernel (sw.hip) share: the
// class geometry, the encoded proteome set, the 64-bit selection key and the host half that turns keys into the hit table.  The
// rule is in include/peprml.h ("Homology search").  Plain C++ outside hipcc; no HIP include.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct pml_sw_opts;
struct pml_proteome_set;
struct pml_sw_result;

namespace pml {

constexpr int SW_CLASSES = 3;
constexpr int SW_STRIP = 8;                    // T: consecutive query rows a lane keeps in registers
constexpr int SW_LANES[SW_CLASSES] = {16, 32, 64};   // lanes of a group; the widest class takes any length in passes of 64 x T rows
constexpr int SW_THREADS = 256;                // a workgroup: 256 / lanes groups, all on the same chunk
constexpr int SW_MARK = 24;                    // the stream's boundary code behind every subject (residue codes are 0 .. 22)
constexpr int SW_PAD_ROW = 24;                 // table row of a query row past the query's end: all zero
constexpr int SW_TROWS = 25, SW_TSTRIDE = 32;  // the table in LDS: int8[25][32], as pairscore.hip pads it
constexpr int SW_BIG = 1 << 28;                // what a boundary step subtracts: larger than any score (65 535 x 127)
constexpr int SW_CHUNK_DEFAULT = 8192;         // stream bytes of a chunk (residues and boundary codes); one longer subject is a chunk alone
constexpr int SW_MAX_LEN = 65535;
constexpr long long SW_UNIT_CELLS_DEFAULT = 1LL << 37;

struct SwOpts { int open, ext; double lambda, K, evalue; bool traceback; int table[576]; };
// false with a message: a negative cost, hits_per_query other than 0 / 1, a table entry outside int8
bool sw_resolve(const pml_sw_opts *o, SwOpts &r, std::string &err);

// every protein of the call, encoded once: codes packed back to back
struct SwSet {
    int G = 0, np = 0;
    std::vector<int> genome_off;               // [G + 1] into proteins
    std::vector<int> genome_of, pos_in_genome; // [np]
    std::vector<long long> off;                // [np + 1] into codes
    std::vector<uint8_t> codes;
    std::vector<std::string> label;
    std::vector<long long> genome_res;         // [G] total residues: N of the E-value
    int len(int p) const { return (int)(off[(size_t)p + 1] - off[(size_t)p]); }
};
bool sw_encode(const pml_proteome_set *set, SwSet &s, std::string &err);
// one residue text -> codes (upper-cased, J O U -> X); -1 and the position of the first other byte
int sw_encode_residues(const char *text, size_t n, uint8_t *out, long long *bad_pos);

inline unsigned long long sw_key(int score, int pos) { return ((unsigned long long)(unsigned)score << 32) | (0xFFFFFFFFull - (unsigned)pos); }
inline int sw_key_score(unsigned long long k) { return (int)(k >> 32); }
inline int sw_key_pos(unsigned long long k) { return (int)(0xFFFFFFFFull - (k & 0xFFFFFFFFull)); }

// the rule's score of one pair in plain loops, row by row
int sw_score_host(const uint8_t *q, int m, const uint8_t *t, int n, const SwOpts &o);
// best[q * G + g] (0 = no subject) -> statistics, cutoff, table text and, if asked for, the traceback; fills res (malloc'ed)
int sw_finish(const SwSet &s, const SwOpts &o, const std::vector<unsigned long long> &best, long long cells, pml_sw_result *res, std::string &err);
long long sw_total_cells(const SwSet &s);

// the raw scores of n encoded sequences against each other through the search's launch path (sw.cpp, the driver under
// pml_debug_sw_scores): scores[a * n + b] = a as the query against b as the subject.  The caller holds the context
struct Ctx;
int sw_scores_encoded(Ctx *ctx, const uint8_t *codes, const long long *off, const int *len, int n, const SwOpts &o, std::vector<int> &scores);

}  // namespace pml
