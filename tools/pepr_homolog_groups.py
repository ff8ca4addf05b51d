#!/usr/bin/env python
"""PEPR's homolog-group step (PhyloPipeline.java:357-406) on the GPU engine: from the all-vs-all hit table to the set files.

usage: pepr_homolog_groups.py -homology_search_method HITS.m8|blast -genome_file FASTA [FASTA ...] [-bidirectional true] [-inflation 1.5]
                              [-run_name NAME] [-out_dir DIR] [-min_taxa N] [-max_taxa N] [-rep_only true] [-target_ntax N]
                              [-target_min_gene N] [-evalue 0.1] [-device 0]
-homology_search_method  the tabular hit table (12 fields a line; the score is field 11), in place of the search the Java runs; or
                         `blast` (HandyConstants.BLAST): the table is first made from the genome files by the exhaustive
                         Smith-Waterman search (tree_builder.HomologySearch, -evalue 0.1) as <run_name>_all_blast.out in -out_dir
                         (default: the working directory)
-bidirectional           filterForBidirectional (:911-987) instead of filterHitPairFile (:989-1024)
-inflation               mcl's -I
Written, under the Java's names: HITS.m8_filtered or HITS.m8_bidir, <that>_mclOut (one cluster per line, labels joined by tabs), and
hg_<run_name>/set_<k>.faa for every line k of it, in -out_dir (default: beside the hit table).  With -min_taxa ... the sets that
createInputSequenceSetProvider (PhylogenomicPipeline2.java:564-605) keeps are listed on stdout.
Clusters and their order equal mcl 09-308's on the committed cases (tests/golden/mcl_cases.json); mcl's selection and recovery
pruning, which act on columns of more than 1100 entries, are not built (include/peprml.h).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine, tree_builder


BLAST = "blast"         # HandyConstants.BLAST


def parse_args(argv):
    """CommandLineProperties style: -flag value [value ...]; a flag without a value is true"""
    args, i = {}, 0
    while i < len(argv):
        if argv[i].startswith("-") and not argv[i][1:2].isdigit():
            key = argv[i].lstrip("-")
            vals = []
            i += 1
            while i < len(argv) and not (argv[i].startswith("-") and not argv[i][1:2].isdigit()):
                vals.append(argv[i])
                i += 1
            args[key] = vals or ["true"]
        else:
            i += 1
    return args


def main(argv=None, ctx=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if "homology_search_method" not in args:
        sys.stderr.write(__doc__)
        return 2
    one = lambda k, d: args.get(k, [d])[0]      # noqa: E731
    ctx = ctx or engine.Context(int(one("device", "0")))
    hits = one("homology_search_method", None)
    if hits == BLAST:
        search = tree_builder.HomologySearch(args.get("genome_file", []), evalue=float(one("evalue", "0.1")), run_name=one("run_name", "run"), ctx=ctx,
                                             out_dir=one("out_dir", "."))
        hits = search.getResults()
        print("%d hits -> %s" % (len(search.result["query"]), hits))
    hg = tree_builder.HomologGroups(hits, args.get("genome_file", []), ctx=ctx,
                                    run_name=one("run_name", "run"), out_dir=args.get("out_dir", [None])[0],
                                    bidirectional=one("bidirectional", "false").lower() == "true", inflation=float(one("inflation", "1.5")),
                                    min_taxa=int(one("min_taxa", "0")), max_taxa=int(one("max_taxa", str(2 ** 31 - 1))),
                                    rep_only=one("rep_only", "false").lower() == "true", target_ntax=int(one("target_ntax", "0")),
                                    target_min_gene=int(one("target_min_gene", "0")))
    r = hg.run()
    print("%d sequences, %d components, %d clusters, %d iterations -> %s" % (len(r["labels"]), r["components"], len(r["clusters"]), r["iterations"], hg.mcl_file))
    if "min_taxa" in args or "max_taxa" in args or "rep_only" in args or "target_ntax" in args:
        for path in hg.getSelectedSetFiles():
            print(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
