#!/usr/bin/env python
"""Developer census on the CPU simulator: which alignments of a region repeat an earlier one of the same region (rtk_pair_note, csrc/hip/rtk_sim_census.h). Per call
site: calls and 32-bit word-columns, and of them those whose (query, target) pair was swept before exactly, transposed, with a query that is a prefix of the
other's on the same target, or with a query of the same length at Hamming distance 1..8 on the same target (the first class that holds). The strings are the
swept ones: a trim by column counts as (corrected, raw). Usage: sim_pairs.py PREFIX [max_reads]"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ratatosk_amd import api
from oracle import oracle_py as op
lib = os.path.join(ROOT, "tests", "hostsim", "librtk_hostsim.so")
L = api.load_library(lib)
pre = sys.argv[1]; mx = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 30
g = api.Graph(pre + ".index.k31.fasta.gz", pre + ".index.k31.rtsk", 31, device=0, lib_path=lib)
reads = op.read_fastq(pre + ".lr.fq")[:mx]
seqs, quals = [r[1] for r in reads], [r[2] for r in reads]
buf = (C.c_ulonglong * 320)()
L.rtk_sim_pair_stats(buf, 1); L.rtk_sim_pairs(1)
b = api.Batch(g, seqs, quals); b.run(g.opts()); st = b.stats(); b.close()
L.rtk_sim_pairs(0); L.rtk_sim_pair_stats(buf, 0)
names = {0: "other", 1: "score terminal NW", 2: "score nonterm HW (ref in path)", 3: "score nonterm HW (path in ref)", 4: "path qual SHW path", 5: "explore prefix SHW", 6: "select nt HW", 7: "resize SHW", 8: "fixRepeats NW", 9: "fixRepeats NW k", 10: "final select NW", 11: "partial select SHW (restart)", 12: "partial select SHW (final)", 13: "trim SHW", 14: "consensus fw NW path", 15: "consensus bw NW path", 16: "consensus final NW", 17: "fixAmbiguity SHW path", 18: "trim by column, stored (fw gap)", 19: "trim by column"}
classes = ("exact", "transposed", "prefix", "hamming 1-8")
tot_calls, tot_cols = sum(buf[10 * i] for i in range(32)), sum(buf[10 * i + 1] for i in range(32))
print("reads %d bases %d regions %d; alignments noted %d, word-columns %d (cols32); fixAmbiguity linked-allele searches run %d skipped %d entries %d" % (
    len(reads), st["in_bases"], st["n_regions"], tot_calls, tot_cols, st["n_fa_linked_run"], st["n_fa_linked_skipped"], st["n_fa_linked_entries"]))
print("per site: calls, cols32 (share of all); then per class: calls / cols32 (share of ALL word-columns)")
for i in range(32):
    c, w = buf[10 * i], buf[10 * i + 1]
    if c:
        print("site %2d %-32s calls %7d cols32 %10d (%.3f) | " % (i, names.get(i, "?"), c, w, w / max(1, tot_cols)) +
              "  ".join("%s %d / %d (%.3f)" % (nm, buf[10 * i + 2 * (j + 1)], buf[10 * i + 2 * (j + 1) + 1], buf[10 * i + 2 * (j + 1) + 1] / max(1, tot_cols)) for j, nm in enumerate(classes)))
for j, nm in enumerate(classes):
    print("all sites, %-12s calls %7d cols32 %10d (%.3f of all word-columns)" % (nm, sum(buf[10 * i + 2 * (j + 1)] for i in range(32)), sum(buf[10 * i + 2 * (j + 1) + 1] for i in range(32)),
                                                                           sum(buf[10 * i + 2 * (j + 1) + 1] for i in range(32)) / max(1, tot_cols)))
