#!/usr/bin/env python
"""TreeComparison's command line (.../pepr/tree/TreeComparison.java:33-199) on the GPU engine.

usage: pepr_tree_compare.py -tree_file FILE [FILE ...] [-rf true] [-tree_dist true] [-use_lengths true]
                            [-outgroup FASTA ...] [-consel true -alignment FILE [-ml_matrix PROTGAMMAWAG]] [-device 0]
-tree_file    files of Newick trees, one tree per non-empty line (:63-79); all trees of all files form one set
-rf           (default true) compare every pair (compareAllvsAll :267-288) and print the Java's lines per pair i < j:
                  i vs j: <legacy RF>
                  Tree Distance: i vs j\\t RF: <legacy RF>\\tBranch Dist: <getBranchDistance>\\t\\t<getDiscrepantBranchDistance>
-tree_dist    (default true) the Java reads this flag (:50) and never uses it: both lines hang on -rf.  Here false drops the
              second line, and the two distances are then not computed.
-use_lengths  (default true) false reads every branch length as 0 (the distances are then NaN, as in the Java)
-outgroup     FASTA files whose sequence titles name taxa to remove from every tree first (:83-99)
Trees over different leaf sets are pruned to their common taxa (:101-128) with the messages the Java prints; the removals
follow BasicTree.removeTaxon (tree_builder.BasicTree).  All values come from ONE pml_tree_compare call.  Doubles are spelled as
everywhere in this project (the shortest text that reads back to the same double: 0 for Java's 0.0, NaN as NaN).
-consel true  the third leg (:149-193): the CONSEL table of the trees on -alignment (FASTA or PHYLIP) under -ml_matrix, through
              pml_tree_tests_weighted and pml_catpv_table (tree_builder.TreeComparison.runConsel)
compareBranchSupports (-support_reps, :139-142) is not built.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine, tree_builder


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


def flag(args, key, default):
    return args.get(key, [default])[0].lower() == "true"


def fasta_titles(path):
    return [line[1:].split()[0] for line in open(path) if line.startswith(">") and len(line) > 1]


def read_alignment(path):
    text = open(path).read()
    names, rows = [], []
    if text.startswith(">"):
        for line in text.splitlines():
            line = line.strip()
            if line.startswith(">"):
                names.append(line[1:].split()[0])
                rows.append([])
            elif line:
                rows[-1].append(line)
        return names, ["".join(r) for r in rows]
    lines = [x for x in text.splitlines() if x.strip()]
    for line in lines[1:1 + int(lines[0].split()[0])]:             # sequential PHYLIP: name, blank, sequence
        parts = line.split()
        names.append(parts[0])
        rows.append("".join(parts[1:]))
    return names, rows


def compare_lines(r, ntrees, tree_dist=True):
    """the lines of compareAllvsAll (:277-282) from the arrays of Context.tree_compare"""
    f = engine.format_double
    out = []
    for i in range(ntrees):
        for j in range(i + 1, ntrees):
            rf = int(r["rf_legacy"][i][j])
            out.append("%d vs %d: %d" % (i, j, rf))
            if tree_dist:
                out.append("Tree Distance: %d vs %d\t RF: %d\tBranch Dist: %s\t\t%s" % (i, j, rf, f(r["branch_dist"][i][j]), f(r["discrepant_dist"][i][j])))
    return out


def main(argv, ctx=None, out=print):
    args = parse_args(argv)
    if "tree_file" not in args:
        raise SystemExit(__doc__)
    use_lengths = flag(args, "use_lengths", "true")
    trees = []
    for i, name in enumerate(args["tree_file"]):
        out("treeFile %d: %s" % (i, name))
        trees += [line.strip() for line in open(name) if line.strip()]
    outgroup = sorted({t for f in args.get("outgroup", []) for t in fasta_titles(f)})
    for t in outgroup:
        out(t)
    trees, removed = tree_builder.pruneToCommonTaxa(trees, outgroup, use_lengths)
    for i, taxon in removed:
        out("tree %d removing taxon: %s" % (i, taxon))
    out("done parsing")
    if ctx is None:
        ctx = engine.Context(int(args.get("device", ["0"])[0]))
    if flag(args, "rf", "true"):
        tree_dist = flag(args, "tree_dist", "true")
        r = ctx.tree_compare(trees, use_lengths=use_lengths, want=None if tree_dist else ["rf_legacy"])
        for line in compare_lines(r, len(trees), tree_dist):
            out(line)
    if flag(args, "consel", "false"):
        aln_file = (args.get("alignment") or args.get("align_file") or [None])[0]
        if aln_file is None:
            raise SystemExit("-consel true needs -alignment FILE")
        names, rows = read_alignment(aln_file)
        keep = [k for k, n in enumerate(names) if n not in outgroup]
        aln = tree_builder.SequenceAlignment([names[k] for k in keep], [rows[k] for k in keep])
        tc = tree_builder.TreeComparison(ctx=ctx, weighted=True)
        out("Results:")
        for line in tc.runConsel(aln, trees, matrix=args.get("ml_matrix", ["PROTGAMMAWAG"])[0]):
            out(line)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
