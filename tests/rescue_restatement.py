"""Restatement of the unmapped-read rescue (`correct -u`, DESIGN.md section 4 [A11]) for tests/test_rescue_reads.py, independent of the C++ and HIP code:
sets of canonical k-mers (A=0 C=1 G=2 T=3, first base in the high bits, the smaller of a k-mer and its reverse complement), computed with numpy.

  LR2 / SR2   canonical k-mers seen at least twice in the long reads / in the -s reads
  a -u read qualifies when, upper-cased, it has at least T = 31 start positions whose k characters are all A/C/G/T and whose canonical k-mer is in
  LR2 and not in SR2 (positions are counted, not distinct k-mers)
  output: ">NAME\\nSEQ\\n" per kept read, SEQ upper-cased, input order; NAME = the header up to its first white space
"""
import gzip

import numpy as np

T = 31

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i


def read_fastx(path):
    """[(name, sequence)] of a FASTA or FASTQ file (plain or gzip); FASTQ records on four lines, FASTA sequences on any number of lines."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)  # (every member of a blocked gzip file)
    lines = raw.decode().split("\n")
    out, i = [], 0
    while i < len(lines):
        ln = lines[i]
        if ln.startswith("@"):
            out.append((ln[1:].split()[0] if ln[1:].split() else "", lines[i + 1].rstrip("\r")))
            i += 4
        elif ln.startswith(">"):
            name = ln[1:].split()[0] if ln[1:].split() else ""
            i += 1
            parts = []
            while i < len(lines) and not lines[i].startswith(">"):
                parts.append(lines[i].rstrip("\r")); i += 1
            out.append((name, "".join(parts)))
        else:
            i += 1
    return out


def position_kmers(seqs, k):
    """(canonical k-mer of every start position of the upper-cased reads laid end to end with a separator, whether its window is all A/C/G/T,
    first position of every read). Positions whose window is not valid hold an arbitrary value."""
    text = "\n".join(s.upper() for s in seqs) + "\n"
    codes = _CODE[np.frombuffer(text.encode("latin-1"), dtype=np.uint8)]
    n = len(codes)
    starts = np.zeros(len(seqs), dtype=np.int64)
    if len(seqs) > 1:
        starts[1:] = np.cumsum([len(s) + 1 for s in seqs[:-1]])
    if n < k:
        return np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool), starts
    m = n - k + 1
    bad = np.concatenate(([0], np.cumsum(codes >= 4)))
    valid = np.zeros(n, dtype=bool)
    valid[:m] = (bad[k:] - bad[:m]) == 0
    c = (codes & 3).astype(np.uint64)
    fw = np.zeros(m, dtype=np.uint64)
    rc = np.zeros(m, dtype=np.uint64)
    for j in range(k):  # base j of the window: bits 2 (k - 1 - j) of the k-mer, its complement bits 2 j of the reverse complement
        fw |= c[j:j + m] << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - c[j:j + m]) << np.uint64(2 * j)
    can = np.zeros(n, dtype=np.uint64)
    can[:m] = np.minimum(fw, rc)
    return can, valid, starts


def seen_twice(seqs, k):
    """Sorted array of the canonical k-mers that the reads hold at least twice."""
    can, valid, _ = position_kmers(seqs, k)
    u, cnt = np.unique(can[valid], return_counts=True)
    return u[cnt >= 2]


def qualifying_positions(seqs, k, lr2, sr2):
    """(per read: number of start positions whose k-mer is in lr2 and not in sr2; number of positions with an all-A/C/G/T window over all reads)."""
    can, valid, starts = position_kmers(seqs, k)
    d = np.setdiff1d(lr2, sr2, assume_unique=True)
    hit = valid & np.isin(can, d)
    csum = np.concatenate(([0], np.cumsum(hit)))
    ends = np.concatenate((starts[1:], [len(can)])) if len(seqs) else starts
    return (csum[ends] - csum[starts]).astype(np.int64), int(valid.sum())


def keep_mask(seqs, k, lr2, sr2, t=T):
    counts, _ = qualifying_positions(seqs, k, lr2, sr2)
    return [len(s) >= k and int(c) >= t for s, c in zip(seqs, counts)]


def rescue_bytes(records, k, lr2, sr2, t=T):
    """The bytes of OUT_extra_sr.fasta for the -u records [(name, seq)] in input order (b"" = no file)."""
    keep = keep_mask([s for _, s in records], k, lr2, sr2, t)
    return "".join(">%s\n%s\n" % (n, s.upper()) for (n, s), kp in zip(records, keep) if kp).encode()
