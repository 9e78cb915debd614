#!/usr/bin/env python3
"""Which instantiation does each row of the tile families' variant tables launch?

    rocprofv3 --kernel-trace --stats -d OUT -o rows -- python tools/tile_rows.py
    python tools/tile_rows.py --list OUT/.../rows_kernel_trace.csv

The first form launches every row of ``tests/test_gpu_tile_variants.py: ROWS`` once, in one process and in list order, under the
knobs that reach it (no comparison: the GPU test does that).  A name query says ``conv_mfma<1,4,1,4,16>`` whatever the MODE,
PREC, SCHED or OCC argument; the kernel names of a trace carry all template arguments.  The second form prints the tile-family
kernels of such a trace in launch order, one per line: the list of two builds must be the same when only host code changed.
"""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FAMILIES = ("conv_mfma_kernel", "resblock_mfma_kernel", "conv_direct_kernel", "conv_narrow_kernel", "conv_fewrows_kernel")


def launch_rows():
    import torch
    from tests.test_gpu_tile_variants import ROWS, knobs_set, run_row
    for row in ROWS:
        with knobs_set(row[-2]):
            run_row(row)
    torch.cuda.synchronize()
    print(len(ROWS), "rows launched")


def list_trace(path):
    with open(path, newline="") as fh:
        recs = [r for r in csv.DictReader(fh) if any(f in r["Kernel_Name"] for f in FAMILIES)]
    for r in sorted(recs, key=lambda r: int(r["Start_Timestamp"])):
        print(r["Kernel_Name"])


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        list_trace(sys.argv[2])
    elif len(sys.argv) == 1:
        launch_rows()
    else:
        sys.exit(__doc__)
