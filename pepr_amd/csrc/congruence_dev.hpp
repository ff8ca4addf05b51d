// congruence_dev.hpp -- the congruence filter's driver (congruence.cpp) in two halves, for a caller that already holds the genes
// in HBM (trim.cpp's chained call): the plan (taxon union, every gene's rows in ascending union index) and the run on CgGene[].
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "../../include/peprml.h"
#include "api_types.hpp"

namespace pml {

struct CgPlan {
    std::vector<std::string> names;                                   // the sorted union of the genes' names
    std::vector<std::vector<std::pair<int, int>>> order;              // per gene: (union index, row of the gene), ascending; a repeated name: its last row
};
// pml_congruence_costs' checks of the genes, then the plan
int cg_plan(Ctx *ctx, int ngenes, const pml_alignment *genes, CgPlan &plan);
// rules 1 to 6 (include/peprml.h) on genes that are resident in the CgGene layout, rows as plan.order lists them (col_base is
// set here); resident_bytes = what the caller holds in HBM for them, counted against the call's budget.  Caller holds ctx->c.mu
int cg_costs_resident(pml_ctx *ctx, const CgPlan &plan, const std::vector<CgGene> &genes, size_t resident_bytes, pml_congruence_result *result);

}  // namespace pml
