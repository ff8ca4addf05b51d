// nj.hpp -- the reference's neighbor-joining path restated on the host (nj.cpp): 24-code alignment bytes, the BLOSUM62 table
// as AlignmentUtilities leaves it, TreeBuilder.getNJTreeString and TreeBuilder.getNJTopology.  No device code, no HIP include.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace pml {

constexpr int NJ_CODES = 24;          // ARNDCQEGHILKMFPSTWYV = 0..19, B 20, Z 21, X 22, '-' and '?' 23
constexpr int NJ_GAP = 23;
enum { NJ_DISTANCE = 0, NJ_SIMILARITY = 1 };

// AlignmentUtilities.convertAminaAcidSequenceToInts (:174-342) for one row of n chars.  The Java DROPS any other byte and
// shifts the rest of the row; that is not reproduced: -1 is returned with the column and the byte of the first one.
int nj_encode24(const char *row, int n, uint8_t *out, int *bad_col, int *bad_byte);
// loadScoringMatrixFromResource("BLOSUM62") (:371-398): rows / columns 0..22 hold the first 23 rows / columns of the file
// (order A..V B J Z X *), row and column 23 stay 0
void blosum62_as_loaded(int table[NJ_CODES * NJ_CODES]);
// TreeBuilder.getNJTreeString (:152-344) and getNJTopology (:34-140) as loops; m is n x n, row major.  false + err: n < 4, or
// no pair passes the strict comparison (where the Java indexes with -1)
bool nj_tree_string(int n, const std::vector<std::string> &names, const double *m, int matrix_type, std::string &out, std::string &err);
bool nj_topology(int n, const std::vector<std::string> &names, const double *m, int matrix_type, std::string &out, std::string &err);
// a double as text that reads back to the same bits (the shortest of %.15g, %.16g, %.17g that does)
std::string nj_number(double x);

}  // namespace pml
