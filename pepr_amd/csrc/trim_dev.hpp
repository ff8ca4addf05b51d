// trim_dev.hpp -- what the two trimmers' host halves (trim.cpp, gblocks.cpp) share, and the block trimmer's sub-batch for the
// caller that chains the stages in HBM (pml_trim_pipeline, trim.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "congruence_dev.hpp"

namespace pml {

constexpr size_t TRIM_BATCH_SLACK = 16 * 256;      // a sub-batch's shared arrays' own alignment
int trim_check_gene(Ctx *ctx, const pml_alignment &A, int g);
size_t trim_hbm_budget(Ctx *ctx);                  // 0.85 of free HBM, or PML_HBM_BUDGET_MB
int trim_gather_tiles(int ntax, size_t ld_out);    // k_colgather workgroups of one gene
int trim_result_alloc(pml_trim_result *res, int ngenes);
// gene g of a result: rows = the trimmed matrix on the host, row p (ld_out bytes apart) = input row rowsrc[p]
int trim_fill_gene(pml_trim_result *res, int g, int ntax, int ncols, long long gom, const std::vector<int> &kept, const std::vector<int> &rowsrc,
                   const char *rows, size_t ld_out);

// a gene that an earlier stage left in HBM: rows ld bytes apart, the first nmap of them the congruence plan's (map: their union indices)
struct TrimResident { const uint8_t *bytes; const uint16_t *map; int nmap, ncols; size_t ld; };

// what one gene adds to a block-trimming sub-batch's allocation
size_t gb_gene_cost(int ntax, int ncols, bool with_map);

// genes[first .. first + count) through k_gbclass, k_gbselect and k_colgather in ONE allocation, no host step between the launches
struct GbBatch {
    Ctx *ctx = nullptr;
    int ng = 0, first = 0;
    std::vector<int> ntax, nmap, ncols, nkept;
    std::vector<std::vector<int>> rowsrc, kept;    // per gene: input row of every uploaded row; kept columns, ascending
    std::vector<size_t> ld, ld_out, o_bytes, o_map, o_out;
    std::vector<long long> gom;
    std::vector<uint8_t> flags;                    // class and stage bytes as the kernels wrote them
    std::vector<char> out_host;
    size_t bytes = 0, out0 = 0;
    char *d = nullptr;
    ~GbBatch();
    // plan: rows in the plan's order, with the map (a congruence stage follows); download: the trimmed matrices come back
    int run(const pml_alignment *genes, int first_, int count, const pml_gblocks_params *params, const CgPlan *plan, bool download);
    int fill(pml_trim_result *res) const;
};

}  // namespace pml
