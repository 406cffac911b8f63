#!/usr/bin/env python3
"""Scores of every ``*_ours.ply`` / ``*_fsct.ply`` pair of a directory against their ``truth`` column on the GPU - the reference's
``pointstowood/comparetofsct.py``.

``python comparetofsct.py DIR``

For both files of a pair: the points labelled 2 are left out, the fsct file's label becomes ``label == 3`` when more than two
distinct labels remain, and precision, recall, balanced accuracy and ``pathlength``-weighted balanced accuracy of ``label`` against
``truth`` are computed (weight 1 without a ``pathlength`` column).  ``DIR/results.csv`` holds the mean per country (the file name's
first three characters) in the reference's layout, ``DIR/results_files.csv`` the unrounded values per file.  The reference's PNG
table is not written.
"""
from __future__ import annotations

import argparse
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    p = argparse.ArgumentParser(description="Precision, recall and balanced accuracy of *_ours.ply / *_fsct.ply pairs against truth.")
    p.add_argument("directory", help="directory holding <name>_fsct.ply and <name>_ours.ply files with truth and label columns")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not os.path.isdir(args.directory):
        raise SystemExit(f"{args.directory}: no such directory")
    if not glob.glob(os.path.join(args.directory, "*_fsct.ply")):
        raise SystemExit(f"{args.directory}: no *_fsct.ply file")
    from pointstowood_amd.evaluate import compare_directory
    try:
        rows = compare_directory(args.directory, verbose=True)
    except ValueError as e:
        raise SystemExit(str(e))
    print(f"{len(rows)} pairs -> {os.path.join(args.directory, 'results.csv')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
