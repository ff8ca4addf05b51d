#!/usr/bin/env python
"""PEPR's homology search (PhyloPipeline.runBlast :1061-1077, BlastRunner) on the GPU engine: from genome FASTA files to the
tabular hit table that pepr_homolog_groups.py reads.

usage: pepr_homology_search.py -genome_file FASTA [FASTA ...] [-evalue 0.1] [-traceback true] [-o hits.m8] [-run_name NAME] [-device 0]
-evalue     the cutoff on E = K m N exp(-lambda S) (the Java's evalueCutoff)
-traceback  fill fields 2..9 (identity, length, mismatches, gap openings, coordinates) from one optimal alignment per hit
-o          the table's file (default <run_name>_all_blast.out in the working directory, BlastRunner's name)
Every protein is aligned against every protein of every genome by affine-gap Smith-Waterman (BLOSUM62, 11/1); per query and
target genome the best subject is kept (-v 1 -b 1).  This is the exact search blastall approximates: parity with blastall is
unpinned, and SEG masking, composition-based statistics and the effective-length correction are not built (include/peprml.h).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine, tree_builder
from pepr_homolog_groups import parse_args


def main(argv=None, ctx=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if "genome_file" not in args:
        sys.stderr.write(__doc__)
        return 2
    one = lambda k, d: args.get(k, [d])[0]      # noqa: E731
    search = tree_builder.HomologySearch(args["genome_file"], evalue=float(one("evalue", "0.1")), run_name=one("run_name", "run"),
                                         ctx=ctx or engine.Context(int(one("device", "0"))), traceback=one("traceback", "false").lower() == "true",
                                         result_file_name=args.get("o", [None])[0])
    path = search.getResults()
    print("%d hits, %d cells -> %s" % (len(search.result["query"]), search.result["cells"], path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
