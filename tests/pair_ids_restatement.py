"""The rule of `rtk_build_index --pair-by-name` (DESIGN.md section 4 [A18]) restated from its statement, and the input layouts it exists for.

name_hash: 64-bit FNV-1a over the bytes of the name, then the mixer of the k-mer tables. pair_ids: a dictionary of first appearances -- a hash gets the next id
when it is first seen, every later record of that hash the same id. read_name: what the readers hand over (the header up to the first blank, without a trailing /1
or /2). The splitter turns an interleaved FASTQ (rtk_simulate: mates adjacent, both named alike) into the files a sequencer writes."""
import random

M64 = (1 << 64) - 1


def name_hash(name):
    h = 0xcbf29ce484222325
    for c in name.encode() if isinstance(name, str) else name:
        h = ((h ^ c) * 0x100000001b3) & M64
    for mul in (0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53):
        h ^= h >> 33
        h = (h * mul) & M64
    return h ^ (h >> 33)


def pair_ids(hashes):
    first, ids = {}, []
    for h in hashes:
        ids.append(first.setdefault(h, len(first)))
    return ids, len(first)


def read_name(header):
    name = header.split()[0] if header.split() else ""
    return name[:-2] if len(name) > 2 and name[-2] == "/" and name[-1] in "12" else name


def read_fastq(path):
    """[(header without '@', sequence, quality)] of a 4-line FASTQ file"""
    with open(path) as f:
        lines = f.read().split("\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


def write_fastq(path, records):
    with open(path, "w") as f:
        for name, seq, qual in records:
            f.write("@%s\n%s\n+\n%s\n" % (name, seq, qual))


def split(inter, prefix, slash=False, shuffle_r2=None, keep_interleaved=0, singletons=0, triple=False):
    """The interleaved file `inter` as PREFIX_R1.fq, PREFIX_R2.fq [, PREFIX_R3.fq]: the paths, in the order to give them with -s.
    slash: mates named X/1 and X/2. shuffle_r2: a seed, R2 in another record order than R1. keep_interleaved: that many pairs (the last ones) stay interleaved in a
    third file. singletons: that many pairs lose their second mate. triple: the first mate of the first pair once more at the end of the last file (a name of three
    records)."""
    recs = read_fastq(inter)
    assert len(recs) % 2 == 0 and all(read_name(recs[i][0]) == read_name(recs[i + 1][0]) for i in range(0, len(recs), 2))
    pairs = [(recs[i], recs[i + 1]) for i in range(0, len(recs), 2)]
    third = [m for p in pairs[len(pairs) - keep_interleaved:] for m in p] if keep_interleaved else []
    pairs = pairs[:len(pairs) - keep_interleaved] if keep_interleaved else pairs
    tag = (lambda r, m: (r[0] + "/%d" % m, r[1], r[2])) if slash else (lambda r, m: r)
    r1 = [tag(a, 1) for a, _ in pairs]
    r2 = [tag(b, 2) for i, (_, b) in enumerate(pairs) if not (singletons and i % max(1, len(pairs) // singletons) == 1)]
    if shuffle_r2 is not None:
        random.Random(shuffle_r2).shuffle(r2)
    files = [(prefix + "_R1.fq", r1), (prefix + "_R2.fq", r2)] + ([(prefix + "_R3.fq", third)] if third else [])
    if triple:
        files[-1][1].append(tag(pairs[0][0], 1))
    for path, records in files:
        write_fastq(path, records)
    return [path for path, _ in files]


def predicted_ids(files):
    """the id of every record of `files` in the order given, with its sequence: [(id, sequence)], and the number of ids"""
    recs = [r for path in files for r in read_fastq(path)]
    ids, n = pair_ids([name_hash(read_name(r[0])) for r in recs])
    return [(i, r[1]) for i, r in zip(ids, recs)], n
