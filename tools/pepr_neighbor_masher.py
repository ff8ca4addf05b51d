#!/usr/bin/env python
"""NeighborMasher's command line (.../util/NeighborMasher.java:102-110, :251-279) on the GPU engine.

usage: pepr_neighbor_masher.py -ingroup FASTA [FASTA ...] [-outgroup FASTA ...] [-k 21] [-s 100000] [-outgroup_count 3]
                               [-expand_ingroup 0] [-ingroup_only true] [-outgroup_only true] [-run_name NAME] [-digits 6] [-device 0]
-ingroup         genome files of the ingroup; -outgroup: the pool of candidate genomes
-k, -s           k-mer length and sketch size
-outgroup_count  outgroup candidates to report
-expand_ingroup  target size of the ingroup after adding the closest pool genomes
Each file is one genome, every sequence a record.  A genome's taxon is read from its FIRST title line by
FastaUtilities.getTaxonFromTitle with stripPipeAndSuffix off (main :103), restated below.
Written, as the Java does: <run>_ingroup.txt and <run>_outgroup.txt (one id per line: the part of the taxon name behind "_@_";
the whole name where it has no such part, the Java throws there), <run>_k<k>_s<s>_ingroup_nj.nwk and
<run>_k<k>_s<s>_rooted_nj.nwk under run()'s conditions (both read -expand_ingroup, not the ingroup's size).
The "rooted" file holds the UNROOTED NJ tree with the outgroup taxa first: AdvancedTree.setOutGroup (:637-640) is not built.
Sketches and distances are the published Mash rule on the device; parity with the mash binary is unpinned (include/peprml.h).
-digits 6 (default) feeds the distance as read from mash's text, -digits 0 the double.
-mash, -p, -outgroup_sketch and -auto_adjust are accepted and ignored with a line on stderr (the last is unused in the Java too).
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine, tree_builder

IGNORED = ("mash", "p", "outgroup_sketch", "auto_adjust")
FORBIDDEN = " ():,[]"          # FastaUtilities.forbiddenChars :6-14


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


def flag(args, key):
    return args.get(key, ["false"])[0].lower() == "true"


def taxon_from_title(title):
    """FastaUtilities.getTaxonFromTitle (:51-114) with stripPipeAndSuffix off: the text inside the last pair of square brackets
    (nested ones skipped), else the title without its '>'; '|' becomes '@'; each forbidden character becomes '_' and doubled
    underscores are merged after each"""
    last_close = -1
    for i in range(len(title) - 1, 0, -1):
        if title[i] == "]":
            last_close = i
            break
    depth, match = 0, -1
    for i in range(last_close - 1, -1, -1):
        if title[i] == "]":
            depth += 1
        elif title[i] == "[":
            if depth == 0:
                match = i
                break
            depth -= 1
    if match > -1 and last_close > -1:
        r = title[match + 1:last_close]
    else:
        r = title[1:] if title.startswith(">") else title
    r = r.replace("|", "@")
    for ch in FORBIDDEN:
        r = r.replace(ch, "_").replace("__", "_")
    return r


def read_genome(path):
    """(taxon name, records) of a FASTA file; bytes before the first title line are ignored"""
    title, records, cur = None, [], None
    with open(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if title is None:
                title = line.decode("latin-1")               # getTaxonName :996-999 reads the first line whatever it is
            if line.startswith(b">"):
                cur = []
                records.append(cur)
            elif cur is not None:
                cur.append(line)
    if title is None:
        raise SystemExit("%s is empty" % path)
    return taxon_from_title(title), [b"".join(r) for r in records]


def id_of(taxon):
    parts = taxon.split("_@_")
    return parts[1] if len(parts) > 1 else taxon


def main(argv, ctx=None):
    args = parse_args(argv)
    if flag(args, "h") or not args.get("ingroup"):
        if not flag(args, "h"):
            print("No ingroup genomes have been specified. Specify ingroup genome file names with the option '-ingroup'")
        raise SystemExit(__doc__)
    for key in IGNORED:
        if key in args:
            sys.stderr.write("-%s is ignored: sketches and distances are computed on the device\n" % key)
    k, s = int(args.get("k", ["21"])[0]), int(args.get("s", ["100000"])[0])
    run = args.get("run_name", ["run_%d" % int(time.time() * 1000)])[0]
    nm = tree_builder.NeighborMasher(ctx if ctx is not None else engine.Context(int(args.get("device", ["0"])[0])))
    nm.setMashKmerLength(k)
    nm.setMashSketchSize(s)
    nm.setOutgroupCount(int(args.get("outgroup_count", ["3"])[0]))
    nm.setExpandedIngroupSize(int(args.get("expand_ingroup", ["0"])[0]))
    nm.setIngroupTreeOnly(flag(args, "ingroup_only"))
    nm.setOutgroupOnly(flag(args, "outgroup_only"))
    nm.setRunName(run)
    nm.setDistanceDigits(int(args.get("digits", ["6"])[0]))
    nm.setIngroupGenomes([read_genome(p) for p in args["ingroup"]])
    nm.setOutgroupGenomes([read_genome(p) for p in args.get("outgroup", [])])
    r = nm.run()
    if r["ingroup_tree"] is not None:
        with open("%s_k%d_s%d_ingroup_nj.nwk" % (run, k, s), "w") as f:
            f.write(r["ingroup_tree"])
    with open(run + "_ingroup.txt", "w") as f:
        f.write("".join(id_of(t) + "\n" for t in r["ingroup"]))
    if not flag(args, "ingroup_only"):
        with open(run + "_outgroup.txt", "w") as f:
            f.write("".join(id_of(t) + "\n" for t in r["outgroup"]))
        if r["rooted_tree"] is not None:
            with open("%s_k%d_s%d_rooted_nj.nwk" % (run, k, s), "w") as f:
                f.write(r["rooted_tree"])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
