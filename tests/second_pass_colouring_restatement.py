"""The rule by which the reads of the first pass colour the index of the second ([A14]; csrc/tools/index/colour_filter.hpp), restated in
Python for tests/test_second_pass_colouring.py: the quality byte below which a base is no base, the pre-masked copy of a colouring file that today's code path
turns into the filtered index, and the colour events and coverage of a set of unitigs by a walk over a dictionary of canonical k-mers."""
import random

_COMP = str.maketrans("ACGT", "TGCA")


def c_min(min_conf, max_qual=40):
    """getQual(min_conf, out_qual = 1, max_qual) of the reference (src/Common.hpp:410-418): the double is cut to an unsigned char."""
    return int(min(min_conf, 1.0) * (max_qual - 1) + 34.0) & 0xFF


def mask(seq, qual, q_min):
    """seq with N where the quality byte is below q_min"""
    return "".join("N" if ord(q) < q_min else c for c, q in zip(seq, qual))


def premask(records, q_min, min_len):
    """records (name, seq, qual or None) as the filter sees them, spelled out for a tool that has no filter: masked bases are N; a read below min_len becomes the
    one-base record N / !, which keeps its id and adds nothing. q_min = 0: no base is masked."""
    out = []
    for name, seq, qual in records:
        if len(seq) < min_len:
            out.append((name, "N", None if qual is None else "!"))
        else:
            out.append((name, mask(seq, qual, q_min) if q_min else seq, qual))
    return out


def fastq_text(records):
    return "".join("@%s\n%s\n+\n%s\n" % r for r in records)


def fasta_text(records):
    return "".join(">%s\n%s\n" % (r[0], r[1]) for r in records)


def read_fastq(path):
    lines = open(path).read().split("\n")
    return [(lines[i][1:].split()[0], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def qualities_in_runs(n, q_min, rng, runs=(1, 2, 62, 63, 64, 200)):
    """n quality characters: runs of the given lengths, each of one character out of {q_min - 1, q_min, q_min + 1, '!', 'I'}"""
    alphabet = [chr(q_min - 1), chr(q_min), chr(q_min + 1), "!", "I"]
    out = []
    while len(out) < n:
        out.extend(rng.choice(alphabet) * rng.choice(runs))
    return "".join(out[:n])


def revcomp(s):
    return s.translate(_COMP)[::-1]


def canonical(km):
    rc = revcomp(km)
    return km if km <= rc else rc


def kmer_table(unitigs, k):
    """canonical k-mer -> unitig; the k-mers of the unitigs are distinct (asserted)"""
    table = {}
    for u, s in enumerate(unitigs):
        for i in range(len(s) - k + 1):
            c = canonical(s[i:i + k])
            assert c not in table, "a k-mer lies on two unitigs (or twice on one)"
            table[c] = u
    return table


def colour_walk(table, n_unitigs, k, reads, ids):
    """(sorted distinct events unitig << 32 | id, k-mers mapped per unitig): every window of every read that holds only A, C, G, T looked up"""
    events, cov, memo = set(), [0] * n_unitigs, {}
    for r, rid in zip(reads, ids):
        hits = memo.get(r)
        if hits is None:
            hits = {}
            for i in range(len(r) - k + 1):
                w = r[i:i + k]
                if w.strip("ACGT"):
                    continue
                u = table.get(canonical(w))
                if u is not None:
                    hits[u] = hits.get(u, 0) + 1
            memo[r] = hits
        for u, n in hits.items():
            cov[u] += n
            events.add((u << 32) | rid)
    return sorted(events), cov


def random_dna(n, rng):
    return "".join(rng.choice("ACGT") for _ in range(n))


def seeded(seed):
    return random.Random(seed)
