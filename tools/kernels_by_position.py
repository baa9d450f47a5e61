#!/usr/bin/env python
"""Kernels of a steady-state compute() by their position in it, from a rocprofv3 --kernel-trace rocpd db (the table of
profiles/r12/r12_ab_final.txt and later): average and median duration of the k-th kernel over the compute() calls that consist of
k_icp_* kernels only and have the most common length, and the span from the first kernel's start to the last one's end.
usage: kernels_by_position.py <db>"""
import collections
import sqlite3
import sys

import numpy as np

cur = sqlite3.connect(sys.argv[1]).cursor()
rows = [(s, e, n.replace("void ", "").replace("srrg2amd::", "").replace("(anonymous namespace)::", "").split("(")[0])
        for n, s, e in cur.execute("select name, start, end from kernels order by start")]
ends = [i for i, r in enumerate(rows) if "final" in r[2]]
seqs = [rows[a + 1:b + 1] for a, b in zip(ends[:-1], ends[1:])]
seqs = [sq for sq in seqs if all(r[2].startswith("k_icp_") for r in sq)]
if not seqs:
    sys.exit("no steady-state compute() found")
length = collections.Counter(len(sq) for sq in seqs).most_common(1)[0][0]
seqs = [sq for sq in seqs if len(sq) == length]
print("%d steady-state compute() calls of %d kernels" % (len(seqs), length))
print("pos | kernel | avg us | median us")
for k in range(length):
    d = np.array([(sq[k][1] - sq[k][0]) / 1000.0 for sq in seqs])
    print("%3d | %-44s | %7.2f | %7.2f" % (k, seqs[-1][k][2][:44], d.mean(), np.median(d)))
spans = np.array([(sq[-1][1] - sq[0][0]) / 1000.0 for sq in seqs])
print("span: median %.2f us, min %.2f, mean %.2f" % (np.median(spans), spans.min(), spans.mean()))
