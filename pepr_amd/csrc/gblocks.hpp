// gblocks.hpp -- the block selection behind the reference's `-gblocks_trim` (MSATrimmer.trim, MSATrimmer.java:41-126) as functions
// that the device (k_gbclass, k_gbselect, gblocks.hip) and the host (pml_gblocks_flags_host, gblocks.cpp) both compile: the two
// cannot disagree.  Plain C++ outside hipcc.  The rule is the published one (Castresana 2000 and the program's documentation),
// stated in include/peprml.h; residues are counted by identity.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PML_GB_HD __host__ __device__ __forceinline__
#else
#define PML_GB_HD inline
#endif

namespace pml {

enum { GB_GAPS_NONE = 1, GB_GAPS_HALF = 2, GB_GAPS_ALL = 3 };      // PML_GBLOCKS_GAPS_*; 0 = PEPR's (-b5=h)
// one byte per column: bits 0-1 = class (0 non-conserved, 1 conserved, 2 highly conserved), bit 2 = gap position, bit 4 = selected
// after step 1, bit 5 = after steps 2 and 3, bit 6 = after step 4, bit 7 = kept.  Bit 3 stays 0.
enum { GB_CLASS = 3, GB_GAP_POS = 4, GB_SEL1 = 16, GB_SEL3 = 32, GB_SEL4 = 64, GB_KEPT = 128 };
constexpr int GB_ROUNDS = 5;          // one round of scans per step
constexpr int GB_CHUNK = 256;         // columns per chunk of k_gbselect = its workgroup's width
constexpr int GB_LDS_COLS = 4096;     // genes of up to this many columns keep a round's scan values in LDS (2 ints per column)

struct GbParams { int b1, b2, b3, b4, b0, gaps; };

// PEPR's values for the fields that are 0, then the bounds: 0 = fine, -1 = outside n/2 < b1 <= b2 <= n, b3 >= 0, b4 >= 2, b0 >= 2
inline int gb_resolve(int n, const GbParams *in, GbParams &p) {
    p = in ? *in : GbParams{0, 0, 0, 0, 0, 0};
    if (n < 1) return -1;
    if (p.b1 == 0) p.b1 = (int)std::ceil(n * 0.8);                 // MSATrimmer.java:94-95, in double as the Java
    if (p.b2 == 0) { const int d = (int)(85LL * n / 100); p.b2 = d > p.b1 ? d : p.b1; }
    if (p.b3 == 0) p.b3 = 8;
    if (p.b4 == 0) p.b4 = 10;
    if (p.b0 == 0) p.b0 = 10;
    if (p.gaps == 0) p.gaps = GB_GAPS_HALF;
    if (2LL * p.b1 <= n || p.b1 > p.b2 || p.b2 > n || p.b3 < 0 || p.b4 < 2 || p.b0 < 2) return -1;
    if (p.gaps < GB_GAPS_NONE || p.gaps > GB_GAPS_ALL) return -1;
    return 0;
}

// class byte of a column: gaps = its '-' bytes, top = the largest count of one non-gap byte (any value below b1 stands for any
// other: the class is 0 then), n = the gene's rows
PML_GB_HD unsigned gb_class(int gaps, int top, int n, const GbParams &p) {
    const bool gap_pos = p.gaps == GB_GAPS_NONE ? gaps > 0 : p.gaps == GB_GAPS_HALF ? 2LL * gaps >= n : false;
    const unsigned cls = (gap_pos || top < p.b1) ? 0u : top >= p.b2 ? 2u : 1u;
    return cls | (gap_pos ? (unsigned)GB_GAP_POS : 0u);
}

// Round r = step r.  Every step is a predicate on "index of the previous / next column with property A (and B)": previous = the
// largest such index <= c, -1 when there is none (an inclusive forward max-scan); next = the smallest >= c, L when there is none
// (an inclusive backward min-scan).  gb_round_in: the column's A and B from its byte as the earlier rounds left it;
// gb_round_out: the byte after the round.  During rounds 2 and 3 bit 5 holds step 2's result.
PML_GB_HD void gb_round_in(int r, unsigned f, bool &A, bool &B) {
    const unsigned cls = f & GB_CLASS;
    const bool z = (f & GB_SEL3) && cls == 0;                      // round 4: a selected non-conserved column
    switch (r) {
    case 1: A = cls != 0; B = false; break;                        // the ends of the class-0 run
    case 2: A = cls == 2; B = !(f & GB_SEL1); break;               // a class-2 column nearer than the block's end, on both sides
    case 3: A = !(f & GB_SEL3); B = false; break;                  // the block's ends
    case 4: A = z && (f & GB_GAP_POS); B = !z; break;              // a gap position nearer than the end of the run of z columns
    default: A = !(f & GB_SEL4); B = false; break;                 // the block's ends
    }
}

PML_GB_HD unsigned gb_round_out(int r, unsigned f, int prevA, int prevB, int nextA, int nextB, const GbParams &p) {
    const unsigned cls = f & GB_CLASS;
    switch (r) {
    case 1: return (cls == 0 && nextA - prevA - 1 > p.b3) ? f : f | GB_SEL1;
    case 2: return ((f & GB_SEL1) && prevA > prevB && nextA < nextB) ? f | GB_SEL3 : f;
    case 3: return ((f & GB_SEL3) && nextA - prevA - 1 < p.b0) ? f & ~(unsigned)GB_SEL3 : f;
    case 4: {
        const bool z = (f & GB_SEL3) && cls == 0;
        return ((f & GB_SEL3) && !(z && (prevA > prevB || nextA < nextB))) ? f | GB_SEL4 : f;
    }
    default: return ((f & GB_SEL4) && nextA - prevA - 1 >= p.b4) ? f | GB_KEPT : f;
    }
}

}  // namespace pml
