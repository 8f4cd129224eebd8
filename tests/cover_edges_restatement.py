"""Helper of tests/test_cover_edges.py, not a test: the last block of the reference's first-pass addCoverage, "Covering low coverage edges."
(src/Graph.cpp:3085-3363), restated loop by loop in Python from the rule (DESIGN.md section 4 [A16]). It works from the bytes of an index built WITHOUT
`--cover-edges-from`: the .rtsk gives the colours (global | local) and the `shared` byte, the unitig FASTA the text and the adjacency, the cover file the
sequences. Record (every unitig as stored, the successors of both strands, getNumberSharedPairID < min_cov_vertices), then per sequence map / extend / jump
(findUnitig), then the adjacency test, the bit test and the bit clearing, ids in file order."""
import gzip
import struct

from test_rtsk_format import _decode_12346

COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s[::-1].translate(COMP)


def read_fasta(path):
    """The sequences of a FASTA file (plain or gzip, any number of lines per record), as written."""
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    out, cur = [], None
    for line in raw.decode().split("\n"):
        line = line.strip("\r")
        if line.startswith(">"):
            if cur is not None:
                out.append("".join(cur))
            cur = []
        elif cur is not None:
            cur.append(line)
    if cur is not None:
        out.append("".join(cur))
    return out


def parse_rtsk(path):
    """[{head, kmcov, shared, glob, local, amb, hap, cycles}] of an .rtsk file as rtk_build_index writes it (common/rtsk_io.hpp)."""
    data = open(path, "rb").read()
    p, recs = 0, []

    def pid():
        nonlocal p
        (w,) = struct.unpack_from("<Q", data, p); p += 8
        f = w & 7
        if f == 1:
            return [b for b in range(61) if (w >> (3 + b)) & 1]
        if f == 2:
            return [w >> 3]
        assert f == 3, "a set form the tool does not write"
        n = w >> 3
        ids = _decode_12346(data[p:p + n]); p += n
        return ids

    while p < len(data):
        head = data[p:p + 16]
        kmcov, shared = struct.unpack_from("<QQ", data, p + 16); p += 32
        r = {"head": head, "kmcov": kmcov, "shared": shared, "glob": pid(), "local": pid(), "amb": pid(), "hap": pid()}
        (n,) = struct.unpack_from("<Q", data, p)
        r["cycles"] = data[p + 8:p + 8 + n]; p += 8 + n
        recs.append(r)
    return recs


def idx(c):
    return 1 << "ACGT".index(c)  # getAmbiguityIndex: A 1, C 2, G 4, T 8


def restate(fasta, rtsk, k, cover_files, mcv=2):
    """-> {"added": ids added per unitig (ascending), "recorded", "covered", "ids_added", "low": the byte recorded for every unitig,
           "crossings": [(sequence number, p, u, v, direction, base)] of the adjacent mappings whose bit is set AS RECORDED (before the serial bit walk)}"""
    seqs = read_fasta(fasta)
    recs = parse_rtsk(rtsk)
    assert len(seqs) == len(recs)
    col = [frozenset(r["glob"]) | frozenset(r["local"]) for r in recs]
    n_km = [len(s) - k + 1 for s in seqs]
    heads = {}  # oriented head k-mer -> (unitig, strand)
    place = {}  # oriented k-mer -> (unitig, offset of the k-mer on the forward strand, strand)
    for u, s in enumerate(seqs):
        heads[s[:k]] = (u, True)
        heads[rc(s[-k:])] = (u, False)
        for j in range(n_km[u]):
            w = s[j:j + k]
            place[w] = (u, j, True)
            place[rc(w)] = (u, j, False)

    def mapped_head(u, strand):
        return seqs[u][:k] if strand else rc(seqs[u][-k:])

    def successors(u, strand):
        end = seqs[u][-k:] if strand else rc(seqs[u][:k])
        return [heads[end[1:] + b] for b in "ACGT" if end[1:] + b in heads]

    # ---- record (src/Graph.cpp:3091-3193)
    kht, recorded = {}, 0
    for u in range(len(seqs)):
        head = seqs[u][:k]
        for strand, shift in ((True, 0), (False, 4)):
            for w, w_strand in successors(u, strand):
                if min(len(col[u] & col[w]), mcv) < mcv:
                    kht[head] = kht.get(head, 0) | (idx(mapped_head(w, w_strand)[k - 1]) << shift)
                    recorded += 1
    kht0 = dict(kht)

    # ---- cover (src/Graph.cpp:3195-3362)
    def find_unitig(s, pos):
        """(unitig, strand, len): the k-mer at pos and the consecutive k-mers of s that follow it on the same unitig"""
        hit = place.get(s[pos:pos + k])
        if hit is None:
            return None
        u, dist, strand = hit
        ln = 1
        if strand:
            while dist + ln < n_km[u] and pos + ln + k - 1 < len(s) and s[pos + ln + k - 1] == seqs[u][dist + ln + k - 1]:
                ln += 1
        else:
            while dist - ln >= 0 and pos + ln + k - 1 < len(s) and s[pos + ln + k - 1] == seqs[u][dist - ln].translate(COMP):
                ln += 1
        return u, strand, ln

    next_id = max([max(c) for c in col if c], default=-1) + 1
    added = [[] for _ in seqs]
    covered, crossings, number = 0, [], -1
    for path in cover_files:
        for s in read_fasta(path):
            number += 1
            s = s.upper()
            if len(s) < k:
                continue
            v, pos = [], 0
            while pos + k <= len(s):  # KmerHashIterator: the windows of k bases, one by one
                um = None if set(s[pos:pos + k]) - set("ACGT") else find_unitig(s, pos)
                if um is None:
                    pos += 1
                else:
                    v.append((pos, um))
                    pos += um[2]  # it_kmer_h += um.len - 1, then ++
            for i in range(len(v) - 1):
                (p0, (u, strand, ln)), (p1, (w, w_strand, _)) = v[i], v[i + 1]
                if p1 != p0 + ln:
                    continue
                head = seqs[u][:k]
                if head not in kht:
                    continue
                c = mapped_head(w, w_strand)[k - 1]
                bit = idx(c) << (0 if strand else 4)
                if kht0[head] & bit:
                    crossings.append((number, p1 - 1, u, w, 0 if strand else 1, "ACGT".index(c)))
                if kht[head] & bit:
                    for _ in range(2):
                        added[u].append(next_id)
                        if w != u:
                            added[w].append(next_id)
                        next_id += 1
                    kht[head] &= ~bit
                    covered += 1
    return {"added": added, "recorded": recorded, "covered": covered, "ids_added": 2 * covered, "crossings": crossings, "low": [kht0.get(s[:k], 0) for s in seqs]}
