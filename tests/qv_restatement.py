"""Restatement of the k-mer QV (rtk_qv, DESIGN.md section 4 [A17]) for tests/test_qv.py, independent of the C++ and HIP code. K-mers are coded A=0 C=1 G=2 T=3,
first base in the high bits; canonical = the smaller of a k-mer and its reverse complement.

  windows of a read   start positions whose k characters are all A/C/G/T (either case)
  found               those whose canonical k-mer is in the set
  row                 missing = windows - found, error_rate = 1 - (found / windows)^(1/k), qv = -10 log10(error_rate)
"""
import math

import numpy as np

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def canonical_kmers(text, k):
    """(canonical k-mer of every start position of the text, whether its k characters are all bases): two arrays of len(text) - k + 1 entries (none: empty)."""
    codes = _CODE[np.frombuffer(text.encode("latin-1") if isinstance(text, str) else text, dtype=np.uint8)]
    m = len(codes) - k + 1
    if m <= 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=bool)
    bad = np.concatenate(([0], np.cumsum(codes >= 4)))
    valid = (bad[k:] - bad[:m]) == 0
    c = (codes & 3).astype(np.uint64)
    fw, rc = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
    for j in range(k):
        fw |= c[j:j + m] << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - c[j:j + m]) << np.uint64(2 * j)
    return np.minimum(fw, rc), valid


def kmer_set(seqs, k, min_count=1):
    """Python set of the canonical k-mers that the sequences hold at least min_count times."""
    can, valid = canonical_kmers("\n".join(seqs), k)  # (laid end to end with a separator, which is no base)
    u, cnt = np.unique(can[valid], return_counts=True)
    return set(int(x) for x in u[cnt >= min_count])


def sorted_array(kmers):
    return np.array(sorted(kmers), dtype=np.uint64)


def windows_found(seq, k, kmers):
    """(windows, found) of one read against a set of canonical k-mers (a Python set, or the sorted array of one)."""
    arr = sorted_array(kmers) if isinstance(kmers, (set, frozenset)) else kmers
    can, valid = canonical_kmers(seq, k)
    return int(valid.sum()), int((valid & np.isin(can, arr)).sum())


def cut(length, k, max_piece):
    """[(start, end)] of the pieces of a read of `length` characters: at most max_piece each, overlapping by k - 1, every window whole in exactly one."""
    out, a = [], 0
    while True:
        out.append((a, min(a + max_piece, length)))
        if a + max_piece >= length:
            return out
        a += max_piece - (k - 1)


def row(windows, found, k):
    """(missing, error_rate, qv) as the table holds them: error_rate rounded to six significant digits and qv (from the unrounded rate) to two decimals, as floats;
    the strings "0" / "inf" when nothing is missing and "nan" / "nan" when there is no window."""
    if windows == 0:
        return 0, "nan", "nan"
    if found == windows:
        return 0, "0", "inf"
    e = 1.0 - (found / windows) ** (1.0 / k)
    return windows - found, float("%.6g" % e), float("%.2f" % (-10.0 * math.log10(e) + 0.0))
