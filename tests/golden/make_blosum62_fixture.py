"""Writes tests/golden/blosum62_as_loaded.json: the 24 x 24 score table as the reference's loader leaves it.

Source of the numbers: the BLOSUM62 data file the reference ships (the NCBI matrix at a scale of ln(2)/2 with the J column; rows
and columns A R N D C Q E G H I L K M F P S T W Y V B J Z X *).  The file is DATA the reference's programs read at run time; it is
read here as text, the way AlignmentUtilities.loadScoringMatrixFromResource (AlignmentUtilities.java:371-398) reads it --
tests/nj_ref.py load_scoring_matrix is that loader restated: an int[24][24], rows / columns 0..22 filled from the first 23 lines
and cells, row and column 23 left 0.  The codes run A..V, B, Z, X, gap, so code Z (21) ends up with the file's J line and code X
(22) with the file's Z line; the file's X and * lines are never used.
Run:  python tests/golden/make_blosum62_fixture.py <path to the reference's BLOSUM62 file>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nj_ref  # noqa: E402


def main():
    lines = open(sys.argv[1]).read().splitlines()
    table = nj_ref.load_scoring_matrix(lines)
    out = {"codes": "ARNDCQEGHILKMFPSTWYVBZX-", "file_order": "ARNDCQEGHILKMFPSTWYVBJZX*", "table": table,
           "quirks": {"Z.Z": table[21][21], "Z.E": table[21][6], "X.X": table[22][22], "X.A": table[22][0], "gap.A": table[23][0]},
           "source": "the reference's BLOSUM62 data file read as AlignmentUtilities.loadScoringMatrixFromResource reads it"}
    with open(os.path.join(HERE, "blosum62_as_loaded.json"), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote blosum62_as_loaded.json; quirks", out["quirks"])


if __name__ == "__main__":
    main()
