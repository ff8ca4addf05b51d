// congruence.hpp -- the host half of the congruence filter (congruence_host.cpp): plain C++, no HIP, also built alone
#pragma once
#include <cstddef>
#include <vector>

namespace pml {

// BipartitionSet.setBipartitions (:110-138) on the column counts of the distinct splits (0 = a trivial split, never kept):
// returns the cutoff and the indices of the kept ones in ascending order.  top_n = 4 n.
int cg_kept_set(const int *count, size_t ndistinct, long long top_n, std::vector<size_t> &kept);

// filterForCongruence's selection (:191-195, :474-503); 0, or -1 when p is not positive or the index falls outside the genes
int cg_select(int ngenes, const long long *mean_cost, double trim_percent, int *keep, int *idx_out, long long *max_cost_out);

}  // namespace pml
