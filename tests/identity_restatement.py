"""Restatement of rtk_identity (DESIGN.md section 4 [A19]) for tests/test_identity.py: the truth file, the reverse complement, a plain O(mn) edit distance,
the rows of OUT.identity.tsv and OUT.identity.reads.tsv. Nothing here comes from the tool or the device code. For long pairs the checker is the reference's own
edlib in its default configuration (oracle.oracle_py.ref_edlib, k = -1, NW, no IUPAC table); pairs of at most 2 000 x 2 000 are checked with the DP as well."""
import numpy as np

from oracle import oracle_py as op

HEADER = "file\treads\taligned\tnot_in_truth\tread_bases\ttruth_bases\tdistance\terror_rate\tidentity\tfurther"
READS_HEADER = "file_index\tname\tlength\ttruth_length\tdistance"
DP_MAX = 2000


def parse_truth(path):
    """{name: (record, start, length, reverse?)} of the file rtk_simulate --lr-truth writes."""
    out = {}
    for line in open(path).read().split("\n"):
        if not line:
            continue
        name, rec, start, length, strand = line.split("\t")
        assert strand in "+-" and name not in out
        out[name] = (int(rec), int(start), int(length), strand == "-")
    return out


_COMP = {"A": "T", "T": "A", "C": "G", "G": "C"}


def revcomp(s):
    """A<->T, C<->G, any other byte as it is; reversed."""
    return "".join(_COMP.get(c, c) for c in reversed(s))


def truth_of(records, entry):
    """The truth of a read: its stretch of the upper-cased record, reverse-complemented on '-'."""
    rec, start, length, rev = entry
    s = records[rec].upper()[start:start + length]
    assert len(s) == length
    return revcomp(s) if rev else s


def dp_distance(a, b):
    """Unit-cost global edit distance, row by row: D[i][j] = min(D[i-1][j] + 1, D[i-1][j-1] + (a[i] != b[j]), D[i][j-1] + 1). The third term runs along the row:
    with x[j] the minimum of the first two, D[i][j] = min over c <= j of x[c] + (j - c) = j + the running minimum of x[c] - c."""
    if not a or not b:
        return max(len(a), len(b))
    bb = np.frombuffer(b.encode("latin-1"), dtype=np.uint8)
    j = np.arange(len(b) + 1, dtype=np.int64)
    row = j.copy()
    for i, ch in enumerate(a.encode("latin-1"), 1):
        x = np.empty(len(b) + 1, dtype=np.int64)
        x[0] = i
        x[1:] = np.minimum(row[1:] + 1, row[:-1] + (bb != ch))
        row = np.minimum.accumulate(x - j) + j
    return int(row[-1])


def dp_distance_batch(reads, truths):
    """dp_distance of many pairs whose truths have one length, all pairs a row at a time (a pair's result is read off after its last row)."""
    n, lens = len(truths[0]), np.array([len(r) for r in reads])
    assert all(len(t) == n for t in truths)
    a = np.zeros((len(reads), max(1, lens.max())), dtype=np.uint8)
    for p, r in enumerate(reads):
        a[p, :len(r)] = np.frombuffer(r.encode("latin-1"), dtype=np.uint8)
    b = np.array([np.frombuffer(t.encode("latin-1"), dtype=np.uint8) for t in truths]).reshape(len(truths), n)
    j = np.arange(n + 1, dtype=np.int64)
    row = np.tile(j, (len(reads), 1))
    out = np.where(lens == 0, n, -1)
    for i in range(1, int(lens.max()) + 1):
        x = np.empty_like(row)
        x[:, 0] = i
        x[:, 1:] = np.minimum(row[:, 1:] + 1, row[:, :-1] + (b != a[:, i - 1:i]))
        row = np.minimum.accumulate(x - j, axis=1) + j
        out[lens == i] = row[lens == i, -1]
    return [int(v) for v in out]


def distance(a, b, dp=True):
    """edlib's distance of two upper-cased strings, bytes equal iff identical; the DP agrees wherever it is affordable (dp=False: the caller runs
    dp_distance_batch over its pairs instead)."""
    a, b = a.upper(), b.upper()
    if not a or not b:
        return max(len(a), len(b))
    d = op.ref_edlib(a.encode("latin-1"), b.encode("latin-1"), k=-1, mode=0, iupac=False)[0]
    if dp and len(a) <= DP_MAX and len(b) <= DP_MAX:
        assert dp_distance(a, b) == d, (len(a), len(b), d)
    return d


def figures(dist, truth_bases):
    """error_rate and identity as the table prints them."""
    if truth_bases == 0:
        return "nan", "nan"
    e = dist / truth_bases
    return "%.6g" % e, "%.6f" % (1.0 - e)


def tables(files, records, truth, dist=distance):
    """(OUT.identity.tsv, OUT.identity.reads.tsv, per file the distances of its aligned reads) for files = [(path as given to -l, [(name, sequence)])]."""
    rows, reads, all_d = [HEADER], [READS_HEADER], []
    nearest = {}  # name -> its smallest distance in the nearest earlier file that aligned it
    for f, (path, recs) in enumerate(files):
        aligned = [(n, s) for n, s in recs if n in truth]
        ds = [dist(s, truth_of(records, truth[n])) for n, s in aligned]
        tb, total = sum(truth[n][2] for n, _ in aligned), sum(ds)
        further = "-" if f == 0 else str(sum(1 for (n, _), d in zip(aligned, ds) if n in nearest and d > nearest[n]))
        here = {}
        for (n, _), d in zip(aligned, ds):
            here[n] = min(d, here.get(n, d))
        nearest.update(here)
        e, ident = figures(total, tb)
        rows.append("\t".join([path, str(len(recs)), str(len(aligned)), str(len(recs) - len(aligned)), str(sum(len(s) for _, s in aligned)), str(tb), str(total), e, ident, further]))
        reads += ["%d\t%s\t%d\t%d\t%d" % (f, n, len(s), truth[n][2], d) for (n, s), d in zip(aligned, ds)]
        all_d.append(ds)
    return "\n".join(rows) + "\n", "\n".join(reads) + "\n", all_d
