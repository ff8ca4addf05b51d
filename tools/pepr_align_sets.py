#!/usr/bin/env python
"""PEPR's alignment step (PhylogenomicPipeline2.alignAll :701-725, getAlignment :737-806) on the GPU engine: every selected set
file is aligned, all sets in ONE batched call (tree_builder.MultipleSequenceAligner.getMSAs; the rule is in include/peprml.h
"Multiple alignment"; parity with muscle is unpinned).

usage: pepr_align_sets.py -sets hg_<run>/set_*.faa [-genome_file FASTA [FASTA ...]] -o DIR [-gap_open 11] [-gap_extend 1]
                          [-host true] [-device 0]
-sets         the set files pepr_homolog_groups.py wrote (FASTA, unaligned proteins)
-genome_file  the genome files of the run: the rows are then titled by taxon, as pepr_homolog_groups.py derives taxa -- the text of
              the last [...] of a sequence's title, or `file <i>` for a sequence of the i-th genome file whose title has none --
              with blanks as `_`, so that pepr_tree_step.py -alignment_dir DIR reads the directory unchanged.  Without it the rows
              keep their id tokens
-o            the directory that receives one FASTA alignment per set: <set file's base name>_align.faa
-host         run the host twin (no device)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine, tree_builder
from pepr_homolog_groups import parse_args


def taxon_names(genome_files):
    """id token -> taxon name, as tree_builder.HomologGroups.run derives it (the last file wins)"""
    out = {}
    for fi, path in enumerate(genome_files):
        for token, lines in tree_builder.readFastaRecords(path):
            title = lines[0]
            lb, rb = title.rfind("["), title.rfind("]")
            out[token] = (title[lb + 1:rb] if 0 <= lb < rb else "file %d" % fi).replace(" ", "_")
    return out


def main(argv=None, ctx=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if "sets" not in args or "o" not in args:
        sys.stderr.write(__doc__)
        return 2
    one = lambda k, d: args.get(k, [d])[0]      # noqa: E731
    host = one("host", "false").lower() == "true"
    if not host:
        ctx = ctx or engine.Context(int(one("device", "0")))
    taxa = taxon_names(args["genome_file"]) if "genome_file" in args else None
    sets, names = [], []
    for path in args["sets"]:
        recs = tree_builder.HomologySearch.readGenome(path)
        tokens = [t.split(" ")[0] for t, _ in recs]
        if taxa is not None:
            missing = [t for t in tokens if t not in taxa]
            if missing:
                raise SystemExit("%s: %s is in none of the genome files" % (path, missing[0]))
            tokens = [taxa[t] for t in tokens]
        sets.append(list(zip(tokens, [r for _, r in recs])))
        names.append(os.path.splitext(os.path.basename(path))[0])
    opts = {k: int(one(k, "0")) for k in ("gap_open", "gap_extend") if k in args}
    aligner = tree_builder.MultipleSequenceAligner(ctx=ctx, host=host, **opts)
    alignments = aligner.getMSAs(sets, names=names)
    os.makedirs(one("o", "."), exist_ok=True)
    for a in alignments:
        with open(os.path.join(one("o", "."), a.getName() + ".faa"), "w") as fh:
            for t, r in zip(a.getTaxa(), a.rows):
                fh.write(">%s\n%s\n" % (t, r))
    print("%d sets aligned -> %s" % (len(alignments), one("o", ".")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
