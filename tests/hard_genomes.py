"""Seeded generator of low-complexity, self-similar test genomes (what rtk_simulate never writes): homopolymer runs below, at and above k and 2k,
microsatellites with units of 2..6 bp (one of them (AT)n, its own reverse complement), inverted repeats W + spacer + rc(W) with spacers 0, 1, 7 and 40,
a family of seven diverged copies of a 300 bp element on either strand, heterozygous substitutions AND insertions / deletions of 1..20 bp, and -- the
`dropout` variant -- windows of 200, 600, 1500 and 3000 bp without any short-read coverage.

Every structure is placed by rule (one after each random flank of 800..2000 bp), never by chance, so a set provably holds what its kind names; the
long reads tile both haplotypes and are topped up until every planted structure lies inside at least three of them. The bytes depend on the
arguments alone: every draw comes from splitmix64 in integer arithmetic (no float, no `random` module), so any machine and any Python write the same
files (tests/test_hard_genomes.py pins their SHA-256).

write_set(prefix, ...) writes PREFIX.ref.fa (two haplotypes), PREFIX.sr.fq (interleaved pairs, both mates one name) and PREFIX.lr.fq, the shapes
rtk_build_index and the oracle read, and returns a manifest (structures with their coordinates on both haplotypes, where every long read came from,
which stretch of which raw read lies over which dropout window)."""

_M = (1 << 64) - 1
_COMP = str.maketrans("ACGT", "TGCA")
KINDS = ("homopolymer", "microsatellite", "inverted", "family", "all")
HOMOPOLYMER_LENGTHS = (17, 19, 21, 23, 25, 27, 31, 33, 44, 64, 100)   # below, at (19, 21, 25, 31) and above every k the tests build, and above 2k
MICROSATELLITES = (("AT", 60), (2, 200), (3, 33), (4, 120), (5, 25), (6, 72))  # (unit or unit length, span): from just above k to 200 bp
INVERTED = ((100, 0), (200, 1), (300, 7), (400, 40), (150, 0))  # (|W|, spacer): 0 and an odd one are what the graph code can trip on
FAMILY_COPIES, FAMILY_LEN, FAMILY_DIV_PER_1024 = 7, 300, 27  # a draw in 27 / 1024 positions, a quarter of them the same base again: ~2 % divergence
DROPOUT_WINDOWS = (200, 600, 1500, 3000)
DROPOUT_K = 19  # a pair is removed if it shares a 19-mer with a window: the smallest k the tests build, so no k-mer of any tested k survives


def rc(s):
    return s[::-1].translate(_COMP)


class Rng:
    """splitmix64 (Steele, Lea, Flood 2014): the whole state is one 64-bit integer"""

    def __init__(self, seed):
        self.s = seed & _M

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & _M
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
        return z ^ (z >> 31)

    def below(self, n):
        return self.next() % n  # (bias below 2^-40 for the n used here)

    def seq(self, n):
        out = []
        while n > 0:
            x = self.next()
            m = min(n, 32)
            out.append("".join("ACGT"[(x >> (2 * i)) & 3] for i in range(m)))
            n -= m
        return "".join(out)


def _primitive_unit(r, n):
    """a unit of n bases that is no repetition of a shorter one (so the period of the microsatellite is n)"""
    while True:
        u = r.seq(n)
        if all(u != u[:d] * (n // d) for d in range(1, n) if n % d == 0):
            return u


def _structures(r, kind):
    """[(label, hap1, hap2)] in planting order"""
    out = []
    if kind in ("homopolymer", "all"):
        for i, n in enumerate(HOMOPOLYMER_LENGTHS):
            out.append(("homopolymer_%d" % n, "ACGT"[i & 3] * n, "ACGT"[i & 3] * (n - (0, 1, 3)[i % 3])))
    if kind in ("microsatellite", "all"):
        for i, (u, span) in enumerate(MICROSATELLITES):
            u = u if isinstance(u, str) else _primitive_unit(r, u)
            n = span // len(u) + 1
            out.append(("microsatellite_%s" % u, u * n, u * (n - i % 3)))
    if kind in ("inverted", "all"):
        for wl, sp in INVERTED:
            w = r.seq(wl)
            s = w + r.seq(sp) + rc(w)
            out.append(("inverted_%d_%d" % (wl, sp), s, s))
    if kind in ("family", "all"):
        element = r.seq(FAMILY_LEN)
        for i in range(FAMILY_COPIES):
            c = "".join(("ACGT"[(x >> 10) & 3] if (x & 1023) < FAMILY_DIV_PER_1024 else b) for b, x in ((b, r.next()) for b in element))
            c = rc(c) if i % 3 == 1 else c
            out.append(("family_%d" % i, c, c))
    if kind == "all":
        for w in DROPOUT_WINDOWS:
            s = r.seq(w)
            out.append(("window_%d" % w, s, s))
    # interleave the kinds, so that a long read meets several of them (a stable rule: sort by the position within the kind)
    order, seen = [], {}
    for s in out:
        key = s[0].split("_")[0]
        seen[key] = seen.get(key, 0) + 1
        order.append((seen[key], len(order), s))
    return [s for _, _, s in sorted(order)]


def _het_flank(r, s):
    """second haplotype of a flank: substitutions at 0.2 %, deletions and insertions of 1..20 bp at 0.05 % each (per 2^16: 131, 33, 33)"""
    out, i = [], 0
    while i < len(s):
        x = r.next()
        e = x & 0xFFFF
        if e < 131:
            out.append("ACGT"[("ACGT".index(s[i]) + 1 + (x >> 16) % 3) & 3]); i += 1
        elif e < 164:
            i += 1 + (x >> 16) % 20
        elif e < 197:
            out.append(s[i]); out.append(r.seq(1 + (x >> 16) % 20)); i += 1
        else:
            out.append(s[i]); i += 1
    return "".join(out)


def genome(seed, kind, rounds=1):
    """(hap1, hap2, structures): structures = [(label, (start, end) on hap1, (start, end) on hap2)]"""
    assert kind in KINDS
    r = Rng(seed)
    h1, h2, n1, n2, where = [], [], 0, 0, []
    def flank():
        nonlocal n1, n2
        f = r.seq(800 + r.below(1201)); g = _het_flank(r, f)
        h1.append(f); h2.append(g); n1 += len(f); n2 += len(g)
    for rnd in range(rounds):
        for label, a, b in _structures(r, kind):
            flank()
            where.append((label if rounds == 1 else "%s.%d" % (label, rnd), (n1, n1 + len(a)), (n2, n2 + len(b))))
            h1.append(a); h2.append(b); n1 += len(a); n2 += len(b)
    flank()
    return "".join(h1), "".join(h2), where


_SR_ERRORS = (30900, 54192, 62908, 65071)  # number of substitutions in a 150 bp mate, per 2^16: Binomial(150, 0.005) cut at four


def _short_reads(r, haps, cov=20, length=150):
    """[(mate1, mate2)]: pairs at `cov` per haplotype, insert 400..600, either strand, 0.5 % substitutions"""
    pairs = []
    for h in haps:
        for _ in range(cov * len(h) // (2 * length)):
            ins = 400 + r.below(201)
            st = r.below(len(h) - ins)
            fr = h[st:st + ins]
            if r.next() & 1:
                fr = rc(fr)
            mates = []
            for m in (fr[:length], rc(fr)[:length]):
                x = r.next()
                n_err = sum(1 for t in _SR_ERRORS if (x & 0xFFFF) >= t)
                if n_err:
                    m = list(m)
                    for j in range(n_err):
                        y = r.next()
                        p = y % length
                        m[p] = "ACGT"[("ACGT".index(m[p]) + 1 + (y >> 32) % 3) & 3]
                    m = "".join(m)
                mates.append(m)
            pairs.append(tuple(mates))
    return pairs


def _read_starts(n, length):
    """tiles of stride length / 6 over a haplotype of n bases + one at the end"""
    length = min(length, n)
    starts = list(range(0, n - length + 1, max(1, length // 6)))
    if starts[-1] != n - length:
        starts.append(n - length)
    return starts, length


BURST_LEN, BURST_FACTOR = 900, 4  # a stretch of a long read at four times the error rate (28 %): no exact k-mer for hundreds of bases, work for the 1-edit search
PLAIN_READS, PLAIN_LEN = 4, 450   # reads over plain flank, shorter than the insert size: nothing for phasing() to remove, so pass 2 may skip their alignment.
# (At half the error rate: at 7 % one in three of such short reads has a single cluster of exact k-mers and pass 1 leaves it as it is.)


def _noisy(r, s, burst=None, clean=False):
    """7 % errors (2.5 % substitutions, 2.5 % deletions, 2 % insertions), BURST_FACTOR times as many inside the source range `burst`, half as many in a
    `clean` read; qualities 5..24;
    returns (read, quality, offset in the read of every source position)"""
    out, q, off = [], [], []
    n = 0
    for i, c in enumerate(s):
        x = r.next()
        e = x & 0xFFFF
        if burst and burst[0] <= i < burst[1]:
            e //= BURST_FACTOR
        elif clean:
            e *= 2
        off.append(n)
        if e < 1638:
            out.append("ACGT"[(x >> 16) & 3]); n += 1
        elif e < 3277:
            continue
        elif e < 4588:
            out.append(c); out.append("ACGT"[(x >> 16) & 3]); n += 2
        else:
            out.append(c); n += 1
    off.append(n)
    read = "".join(out)
    while len(q) < len(read):
        x = r.next()
        q.extend(chr(38 + ((x >> (8 * i)) & 0xFF) % 20) for i in range(8))
    return read, "".join(q[:len(read)]), off


def _long_reads(r, haps, structures, length):
    """reads of `length` source bases, alternating haplotypes, every third one reverse-complemented. Every planted structure (dropout windows are no
    structures) ends up inside at least three reads. Every fourth read carries a burst of errors; a few short reads over plain flank come last."""
    plan = []  # (hap, start, end)
    tiles = [_read_starts(len(h), length) for h in haps]
    for j in range(max(len(t[0]) for t in tiles)):
        for hp in (0, 1):  # start j of haplotype j % 2, so the two haplotypes alternate along the genome and the tiling of either is half as dense
            if (j + hp) % 2 == 0 and j < len(tiles[hp][0]):
                plan.append((hp, tiles[hp][0][j], tiles[hp][0][j] + tiles[hp][1]))
    for label, c1, c2 in structures:
        if label.startswith("window"):
            continue
        inside = sum(1 for hp, a, b in plan if a <= (c1, c2)[hp][0] and (c1, c2)[hp][1] <= b)
        while inside < 3:
            hp = inside % 2
            ln = min(length, len(haps[hp]))
            mid = ((c1, c2)[hp][0] + (c1, c2)[hp][1]) // 2
            a = max(0, min(len(haps[hp]) - ln, mid - ln // 2 + 97 * inside))
            assert a <= (c1, c2)[hp][0] and (c1, c2)[hp][1] <= a + ln, "long reads too short for " + label
            plan.append((hp, a, a + ln)); inside += 1
    # reads over plain flank: the middle of the flank before each of the first PLAIN_READS structures, haplotypes alternating
    for i, (label, c1, c2) in enumerate(structures[1:1 + PLAIN_READS]):
        hp = i % 2
        mid = (structures[i][1 + hp][1] + (c1, c2)[hp][0]) // 2
        plan.append((hp, mid - PLAIN_LEN // 2, mid - PLAIN_LEN // 2 + PLAIN_LEN))
    reads = []
    for i, (hp, a, b) in enumerate(plan):
        src = haps[hp][a:b]
        burst = (len(src) // 3, len(src) // 3 + BURST_LEN) if i % 4 == 1 and len(src) >= 3 * BURST_LEN else None  # every fourth read of 2.7 kb and more
        read, q, off = _noisy(r, src, burst, clean=len(src) <= PLAIN_LEN)
        rev = i % 3 == 0
        if rev:
            read, q = rc(read), q[::-1]
        reads.append(dict(name="lr%d" % i, seq=read, qual=q, hap=hp, start=a, end=b, rev=rev, off=off, burst=burst is not None))
    return reads


def _kmers_both_strands(s, k):
    out = set()
    for t in (s, rc(s)):
        for i in range(len(t) - k + 1):
            out.add(t[i:i + k])
    return out


def write_set(prefix, seed, kind, lr_len=3000, rounds=1, dropout=False):
    h1, h2, structures = genome(seed, kind, rounds)
    haps = (h1, h2)
    pairs = _short_reads(Rng(seed * 1000003 + 1), haps)
    if dropout:
        gone = set()
        for label, c1, c2 in structures:
            if label.startswith("window"):
                gone |= _kmers_both_strands(h1[c1[0]:c1[1]], DROPOUT_K)
        pairs = [p for p in pairs if not any(m[i:i + DROPOUT_K] in gone for m in p for i in range(len(m) - DROPOUT_K + 1))]
    reads = _long_reads(Rng(seed * 1000003 + 2), haps, structures, lr_len)
    with open(prefix + ".ref.fa", "w") as f:
        f.write(">hap1\n%s\n>hap2\n%s\n" % haps)
    with open(prefix + ".sr.fq", "w") as f:
        for i, p in enumerate(pairs):
            for m in p:
                f.write("@sr%d\n%s\n+\n%s\n" % (i, m, "I" * len(m)))
    with open(prefix + ".lr.fq", "w") as f:
        for rd in reads:
            f.write("@%s\n%s\n+\n%s\n" % (rd["name"], rd["seq"], rd["qual"]))
    # which stretch of which raw read lies over which dropout window
    over = []
    for label, c1, c2 in structures:
        if not label.startswith("window"):
            continue
        for i, rd in enumerate(reads):
            a, b = max((c1, c2)[rd["hap"]][0], rd["start"]), min((c1, c2)[rd["hap"]][1], rd["end"])
            if b - a < 1000:
                continue
            x, y = rd["off"][a - rd["start"]], rd["off"][b - rd["start"]]
            if rd["rev"]:
                x, y = len(rd["seq"]) - y, len(rd["seq"]) - x
            over.append((label, i, x, y))
    for rd in reads:
        del rd["off"]
    return dict(haps=haps, structures=structures, reads=reads, n_pairs=len(pairs), over_windows=over)
