"""`rtk_build_index --subsample-colours`: the read ids that colour the graph thinned out by coverage before the colours are final, as the reference's index step
does by default (addCoverage, src/Graph.cpp:2312-2870, with estimateHaplotypeCoverage, src/Graph.cpp:4185-4234; DESIGN.md section 4 [A12]).

The rule is restated here in Python (`_rule`, `_thin`), from those reference lines and the three deviations the tool documents (a hash of the id for the random
draw; exactly min_cov_vertices forced ids per non-branching unitig; integer quantile boundaries) -- not from the tool's code. It starts from the files of a run
WITHOUT the option (unitigs, coverages, colours), rebuilds the adjacency from the sequences and recomputes only what is compared: the colours per unitig and the
counts of the tool's `subsample:` line.

CPU tier: the whole tool, plain and --fast, k = 31 and k = 63; low coverage (nothing subsampled: the files of a run without the option); the rule on crafted
graphs through rtk_subsample_step (the step on unitigs given by hand); the command line. GPU tier: the device route (csrc/hip/rtk_index.hip k_sub_*) through its
stage entry on crafted events, `rtk_build_index --gpu --subsample-colours` against `--fast`, and one `Ratatosk correct -s ... --subsample-colours` against the
oracle's two passes on the index files of the subsampled host build. The complete one-command run needs the device for its index steps, so that both index
steps receive the option and that the run ends with OUT.fastq is held there (test_gpu_one_command_with_subsampled_colours); without a GPU the first child
command is checked."""
import gzip
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import BIN

TOOL = os.path.join(BIN, "rtk_build_index")
STEP = os.path.join(BIN, "rtk_subsample_step")
EXE = os.path.join(BIN, "Ratatosk")
MCV = 2  # min_cov_vertices of the tool
M64 = (1 << 64) - 1

# 60x diploid: a k = 63 k-mer of a 150-base read sees (150 - 62) / 150 of the base coverage and survives a read error rate e with (1 - e)^63
SETS = {
    "het_repeats": ["--seed", "11", "--ref-len", "30000", "--het", "0.004", "--repeat-frac", "0.1", "--sr-cov", "60", "--sr-err", "0.002"],
    "tandem": ["--seed", "21", "--ref-len", "60000", "--het", "0.003", "--tandem", "30", "--sr-cov", "60", "--sr-err", "0.002"],
}
LINE = re.compile(r"rtk_build_index: subsample: hap_cov=(\d+) rate=([0-9.]+) ids=(\d+)->(\d+) events=(\d+)->(\d+) bins=(\d+) sampled_bins=(\d+)")


# ---------------------------------------------------------------------------------------------------------------- the rule, restated
def _h(i, seed):
    z = (i + seed * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _u(i, seed):
    return (_h(i, seed) >> 11) * 2.0 ** -53


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _thin(cols, bin_of, forced, sampled, mcv, rate, seed):
    """colours per unitig -> (new colours per unitig, distinct ids before, after)"""
    first = {}
    for ids, b in zip(cols, bin_of):
        for i in ids:
            first[i] = min(first.get(i, 255), b)
    keep = set()
    for ids, f in zip(cols, forced):
        if f:
            keep.update(ids if len(ids) <= mcv else [i for _, i in sorted((_h(i, seed), i) for i in ids)[:mcv]])
    for i, b in first.items():
        if b != 255 and (not sampled[b] or _u(i, seed) <= rate):
            keep.add(i)
    new = {i: r for r, i in enumerate(sorted(keep))}
    return [[new[i] for i in ids if i in keep] for ids in cols], len(first), len(keep)


def _rule(units, k, mcv, seed):
    """units: [(sequence, coverage, sorted colours)] of a compacted graph. Returns None when nothing is subsampled (H < 10), else a dictionary."""
    n = len(units)
    where = {}
    for u, (seq, _, _) in enumerate(units):
        for p in range(len(seq) - k + 1):
            km = seq[p:p + k]
            where[min(km, _rc(km))] = u

    def successors(u, fw):  # oriented successors of an oriented unitig
        seq = units[u][0] if fw else _rc(units[u][0])
        out = []
        for b in "ACGT":
            y = seq[-k + 1:] + b
            w = where.get(min(y, _rc(y)))
            if w is not None:
                out.append((w, y == units[w][0][:k]))
        return out

    tot_cov = nb_km = 0
    for u in range(n):
        succ = successors(u, True)
        if len(succ) < 2 or any(len(successors(w, f)) > 1 or len(successors(w, not f)) > 1 for w, f in succ):
            continue
        ends = [e for w, f in succ for e in successors(w, f)]
        if any(e != ends[0] for e in ends):
            continue
        for w, _ in succ:
            nb_km += len(units[w][0]) - k + 1
            tot_cov += units[w][1]
    hap = tot_cov // nb_km if nb_km else 0
    if hap < 10:
        return None
    rate = 5.0 / hap
    kc = [int(cov / (len(seq) - k + 1) + 0.5) for seq, cov, _ in units]
    s = sorted(kc, reverse=True)
    p = [n - 1] + [n * (20 - j) // 20 for j in range(1, 21)]
    bins = [(s[p[j]], s[p[j + 1]]) for j in range(20)]
    live = [lo < hi for lo, hi in bins]
    sampled = [live[j] and bins[j][0] >= 5 for j in range(20)]
    bin_of = [next((j for j in range(20) if live[j] and bins[j][0] <= c < bins[j][1]), 255) for c in kc]
    forced = [len(successors(u, True)) <= 1 and len(successors(u, False)) <= 1 for u in range(n)]
    cols, before, after = _thin([c for _, _, c in units], bin_of, forced, sampled, mcv, rate, seed)
    return dict(hap=hap, rate=rate, cols=cols, ids=(before, after), events=(sum(len(c) for _, _, c in units), sum(len(c) for c in cols)), bins=sum(live), sampled_bins=sum(sampled),
                bin_of=bin_of, forced=forced, sampled=sampled)


# ---------------------------------------------------------------------------------------------------------------- helpers
def _simulate(tmp, name, args, lr=("--lr-n", "2", "--lr-len", "1000")):
    pre = os.path.join(tmp, name)
    subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre] + args + list(lr), stderr=subprocess.DEVNULL)
    return pre


def _build(sr, out, k, extra, env=None):
    r = subprocess.run([TOOL, "-s", sr, "-o", out, "-k", str(k), "--snps"] + extra, capture_output=True, text=True, env=dict(os.environ, RTK_INDEX_TRACE="1", **(env or {})))
    assert r.returncode == 0, r.stderr
    return open(out + ".index.k%d.fasta.gz" % k, "rb").read(), open(out + ".index.k%d.rtsk" % k, "rb").read(), r.stderr


def _units(out, k):
    """[(sequence, coverage, colours)] of the index files OUT.index.k<k>.*, by the oracle's readers"""
    from oracle import oracle_py as op
    g = op.Graph(out + ".index.k%d.fasta.gz" % k, out + ".index.k%d.rtsk" % k, k)
    res = []
    for u in range(g.n_unitigs):
        d = g.unitig(u)
        ids = sorted(set(d["local"]) | (set(g.global_set(d["global_id"])) if d["global_id"] >= 0 else set()))
        res.append((d["seq"], (d["kmcov"] >> 31) & 0x7FFFFFFF, ids))
    return res


def _line(stderr):
    m = LINE.search(stderr)
    assert m, stderr
    v = m.groups()
    return dict(hap=int(v[0]), rate=float(v[1]), ids=(int(v[2]), int(v[3])), events=(int(v[4]), int(v[5])), bins=int(v[6]), sampled_bins=int(v[7]))


def _assert_subsampled(line):
    """the run did subsample: a test must not pass on a run that thinned nothing"""
    assert line["hap"] >= 10 and line["ids"][1] < line["ids"][0], line
    assert line["sampled_bins"] >= 1 and line["bins"] - line["sampled_bins"] >= 1, line


def _check_against_the_rule(base, got_out, k, line, seed=1):
    want = _rule(_units(base, k), k, MCV, seed)
    assert want is not None
    got = _units(got_out, k)
    plain = _units(base, k)
    assert [(s, c) for s, c, _ in got] == [(s, c) for s, c, _ in plain]  # unitigs and coverage as they were
    bad = [u for u in range(len(got)) if got[u][2] != want["cols"][u]]
    assert not bad, ("colour sets differ from the restated rule", len(bad), bad[:5])
    assert (line["hap"], line["ids"], line["events"], line["bins"], line["sampled_bins"]) == (want["hap"], want["ids"], want["events"], want["bins"], want["sampled_bins"]), (line, want["ids"], want["events"])
    assert abs(line["rate"] - want["rate"]) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- CPU tier
@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("subsample_sets"))
    return {name: _simulate(tmp, name, args) + ".sr.fq" for name, args in SETS.items()}


@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("name", sorted(SETS))
def test_whole_tool_against_the_restated_rule(reads, tmp_path, name, k):
    tmp, sr = str(tmp_path), reads[name]
    base = os.path.join(tmp, "base")
    a = _build(sr, base, k, [])
    assert "subsample:" not in a[2]  # no option: no step
    b = _build(sr, os.path.join(tmp, "plain"), k, ["--subsample-colours"])
    c = _build(sr, os.path.join(tmp, "fast"), k, ["--fast", "--subsample-colours"])
    line = _line(b[2])
    _assert_subsampled(line)
    assert b[0] == a[0] and b[1] != a[1]
    assert b[0] == c[0] and b[1] == c[1], "plain and --fast differ"
    assert _line(c[2]) == line
    _check_against_the_rule(base, os.path.join(tmp, "plain"), k, line)
    if name == "het_repeats":  # the seed changes the draw, the same seed repeats it
        d = _build(sr, os.path.join(tmp, "seed7"), k, ["--subsample-colours", "--subsample-seed", "7"])
        e = _build(sr, os.path.join(tmp, "seed7b"), k, ["--fast", "--subsample-colours", "--subsample-seed", "7"])
        assert d[1] != b[1] and d[1] == e[1] and d[0] == b[0]
        _check_against_the_rule(base, os.path.join(tmp, "seed7"), k, _line(d[2]), seed=7)
        f = _build(sr, os.path.join(tmp, "seed1"), k, ["--subsample-colours", "--subsample-seed", "1"])
        assert f[1] == b[1]  # (1 is the default)


def test_low_coverage_is_left_alone(tmp_path):
    tmp = str(tmp_path)
    sr = _simulate(tmp, "low", ["--seed", "11", "--ref-len", "30000", "--het", "0.004", "--repeat-frac", "0.1", "--sr-cov", "12", "--sr-err", "0.002"]) + ".sr.fq"
    for mode in ([], ["--fast"]):
        a = _build(sr, os.path.join(tmp, "a"), 31, mode)
        b = _build(sr, os.path.join(tmp, "b"), 31, mode + ["--subsample-colours"])
        m = re.search(r"rtk_build_index: subsample: hap_cov=(\d+) off\n", b[2])
        assert m and int(m.group(1)) < 10, b[2]
        assert a[0] == b[0] and a[1] == b[1]
        assert "subsample:" not in a[2]


def _random_seq(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def _bubble(rnd, k):
    """the four unitigs of a heterozygous SNP: P, the two branches (k k-mers each), S"""
    p, s = _random_seq(rnd, k + 20), _random_seq(rnd, k + 25)
    return [p, p[-(k - 1):] + "A" + s[:k - 1], p[-(k - 1):] + "C" + s[:k - 1], s]


def _step(units, k, seed=1):
    text = "".join("%s %d %s\n" % (seq, cov, " ".join(str(i) for i in ids)) for seq, cov, ids in units)
    outs = []
    for fast in ("0", "1"):
        r = subprocess.run([STEP, str(k), str(seed), fast], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(([[int(x) for x in l.split(":")[1].split()] for l in r.stdout.splitlines()], r.stderr))
    assert outs[0] == outs[1]  # one thread and many: the same
    return outs[0]


def _crafted(rnd, k, covs, colours):
    """a bubble at per-k-mer coverage 20 on both branches (H = 20) and isolated unitigs of 30 k-mers at the per-k-mer coverages `covs` with the given colours"""
    b = _bubble(rnd, k)
    units = [(b[0], 40 * (len(b[0]) - k + 1), list(range(0, 40))), (b[1], 20 * k, list(range(0, 20))), (b[2], 20 * k, list(range(20, 40))), (b[3], 40 * (len(b[3]) - k + 1), list(range(0, 40)))]
    for c, ids in zip(covs, colours):
        units.append((_random_seq(rnd, k + 29), c * 30, sorted(ids)))
    return units


@pytest.mark.parametrize("k", [31, 63])
def test_rule_on_crafted_graphs(k):
    rnd = random.Random(1000 + k)
    rate = 5.0 / 20
    dropped = [i for i in range(1000, 1400) if _u(i, 1) > rate]  # ids that a sampled bin does not keep
    kept = [i for i in range(1000, 1400) if _u(i, 1) <= rate]
    assert len(dropped) > 100 and len(kept) > 20
    # fewer than 20 unitigs (bins empty or repeated); a unitig with exactly mcv and one with mcv + 1 colours; an id (dropped[0]) that colours a low-coverage unitig
    # of a keep-all bin and a high-coverage one of a sampled bin
    covs = [2, 3, 8, 12, 12, 30, 30]
    colours = [[dropped[0], dropped[1], kept[0]], dropped[2:12], dropped[12:12 + MCV], dropped[20:20 + MCV + 1], dropped[30:60] + kept[1:4], [dropped[0]] + dropped[60:90], kept[4:10] + dropped[90:100]]
    units = _crafted(rnd, k, covs, colours)
    assert len(units) < 20
    got, err = _step(units, k)
    want = _rule(units, k, MCV, 1)
    line = _line(err)
    assert want is not None and got == want["cols"], (got, want["cols"])
    assert (line["hap"], line["ids"], line["events"], line["bins"], line["sampled_bins"]) == (20, want["ids"], want["events"], want["bins"], want["sampled_bins"])
    _assert_subsampled(line)
    assert want["sampled"][want["bin_of"][4]] is False and want["sampled"][want["bin_of"][9]] is True
    assert len(got[4]) == 3 and len(got[5]) == 10  # below coverage 5: everything stays
    assert len(got[6]) == MCV  # exactly mcv colours on a non-branching unitig: all forced, though none is drawn
    assert len(got[7]) == MCV  # mcv + 1 colours, none drawn: the mcv of smallest hash
    x = got[4][units[4][2].index(dropped[0])]  # the new id of dropped[0], kept through its keep-all bin (unitig 4 keeps all three) ...
    assert x in got[9] and len(got[9]) < len(units[9][2])  # ... so it stays on the high-coverage unitig of a sampled bin, which loses others
    # every unitig at one coverage: all at the maximum, no bin, only forced ids survive
    units = _crafted(rnd, k, [20] * 6, [dropped[10 * j:10 * j + 10] + kept[j:j + 1] for j in range(6)])
    units = [(s, 20 * (len(s) - k + 1), c) for s, _, c in units]
    got, err = _step(units, k)
    want = _rule(units, k, MCV, 1)
    assert got == want["cols"] and want["bins"] == 0
    assert _line(err)["bins"] == 0 and _line(err)["sampled_bins"] == 0
    assert all(len(c) == MCV for c in got[1:3] + got[4:])
    assert got[0] == got[3] == sorted(got[1] + got[2])  # the branching P and S force nothing: they keep what their branches forced
    # low coverage on the bubble: off, the colours as they were
    units = [(s, c // 3, ids) for s, c, ids in units]
    got, err = _step(units, k)
    assert "hap_cov=6 off" in err and got == [ids for _, _, ids in units] and _rule(units, k, MCV, 1) is None


def test_command_line(tmp_path):
    tmp = str(tmp_path)
    lr = os.path.join(tmp, "lr.fq")
    open(lr, "w").write("@r\nACGT\n+\nIIII\n")
    # handed to the index step (the child command is shown with -v; without a GPU the step then fails and ends the run)
    r = subprocess.run([EXE, "correct", "-v", "-s", os.path.join(tmp, "missing.fq"), "--subsample-colours", "--subsample-seed", "5", "-l", lr, "-o", os.path.join(tmp, "out")], capture_output=True, text=True)
    step1 = [l for l in r.stderr.splitlines() if "step 1" in l and "rtk_build_index" in l and " -s " in l]
    assert r.returncode != 0 and step1 and "--subsample-colours --subsample-seed 5" in step1[0], r.stderr
    r = subprocess.run([EXE, "correct", "-v", "-s", os.path.join(tmp, "missing.fq"), "-l", lr, "-o", os.path.join(tmp, "out")], capture_output=True, text=True)
    assert "--subsample" not in r.stderr
    # not next to a pre-built index
    for extra in (["--subsample-colours"], ["--subsample-seed", "3"]):
        r = subprocess.run([EXE, "correct", "-1", "-g", "a", "-d", "b", "-l", lr, "-o", os.path.join(tmp, "out")] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "--subsample-colours" in r.stderr and "-g" in r.stderr, r.stderr
    # the seed alone switches nothing on, in either program, and has to be a number
    sr = os.path.join(tmp, "missing.fq")
    for cmd in ([EXE, "correct", "-s", sr, "--subsample-seed", "3", "-l", lr, "-o", os.path.join(tmp, "out")], [TOOL, "-s", sr, "--subsample-seed", "3", "-o", os.path.join(tmp, "out")]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode != 0 and "--subsample-seed without --subsample-colours" in r.stderr, r.stderr
    for cmd in ([EXE, "correct", "-s", sr, "--subsample-colours", "--subsample-seed", "x7", "-l", lr, "-o", os.path.join(tmp, "out")], [TOOL, "-s", sr, "--subsample-colours", "--subsample-seed", "7x", "-o", os.path.join(tmp, "out")]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode != 0 and "unsigned number" in r.stderr, r.stderr
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert "--subsample-colours" in r.stderr and "--subsample-seed" in r.stderr
    r = subprocess.run([TOOL], capture_output=True, text=True)
    assert "--subsample-colours" in r.stderr


def test_stage_entry_needs_a_device():
    """the stage entry exists in the library and, like every compute entry, does not fall back to the host"""
    from ratatosk_amd import api
    try:
        out, before, after = api.index_subsample_events([5], 1, [0], [1], [0], 2, 1.0)
    except api.RtkError as e:
        assert "no such HIP device" in str(e)
    else:  # (a machine with a GPU)
        assert out.tolist() == [0] and (before, after) == (1, 1)


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def _events(cols):
    return np.array([(u << 32) | i for u, ids in enumerate(cols) for i in ids], dtype=np.uint64)


def _cases():
    """name -> (colours per unitig, bin of every unitig, forced candidates): the smallest shapes at which the kernels can go wrong"""
    rnd = random.Random(99)
    cases = {}

    def make(name, cols, n_bins=20, bins=None, forced=None):
        cols = [sorted(set(c)) for c in cols]
        cases[name] = (cols, bins if bins is not None else [rnd.choice(list(range(n_bins)) + [255]) for _ in cols], forced if forced is not None else [rnd.randrange(4) != 0 for _ in cols])

    for n in (0, 1, 63, 64, 65, 255, 257, 4097):  # events in all, in segments of random length (some unitigs without any)
        cols, left = [], n
        while left:
            m = min(left, rnd.choice([0, 1, 2, 3, 5, 17, 64, 65, 130]))
            cols.append(rnd.sample(range(3 * n + 10), m)); left -= m
        make("n_events_%d" % n, cols or [[]])
    make("word_edges", [[62, 63, 64, 65, 66], [4094, 4095, 4096, 4097, 4098], [63, 64, 4095, 4096], [0, 127, 128]])
    make("sparse_ids", [[3, 70000001, 100000003], [70000001], rnd.sample(range(100000004), 200)])
    make("segment_lengths", [rnd.sample(range(5000), m) for m in (0, 1, 1, 2, 3, 4, 64, 65, 1000, 0, 2)], forced=[1] * 11)
    make("one_unitig", [rnd.sample(range(9000), 3000)], bins=[7], forced=[1])
    make("one_event_per_unitig", [[rnd.randrange(500)] for _ in range(300)])
    make("no_bin", [rnd.sample(range(300), 40), rnd.sample(range(300), 70), rnd.sample(range(300), 5)], bins=[255, 3, 255], forced=[1, 0, 1])
    make("largest_id", [[0, 5, (1 << 32) - 1], [(1 << 32) - 2, (1 << 32) - 1]], bins=[2, 255], forced=[0, 1])
    return cases


CASES = _cases()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_stage_entry_against_the_restated_rule(name):
    from ratatosk_amd import api
    cols, bin_of, forced = CASES[name]
    ev = _events(cols)
    combos = [(mcv, rate, sampled) for mcv in (1, 2, 3) for rate in (0.0, 0.5, 1.0) for sampled in ("all", "none", "mixed")]
    if name in ("largest_id", "sparse_ids"):  # (tables of gigabytes: a few combinations)
        combos = [(2, 0.5, "mixed"), (3, 0.0, "all"), (1, 1.0, "none")]
    for mcv, rate, which in combos:
        sampled = [1] * 20 if which == "all" else ([0] * 20 if which == "none" else [j % 3 != 0 for j in range(20)])
        for seed in (1, 12345):
            got, before, after = api.index_subsample_events(ev, len(cols), bin_of, forced, sampled, mcv, rate, seed=seed)
            want_cols, w_before, w_after = _thin(cols, bin_of, forced, sampled, mcv, rate, seed)
            want = _events(want_cols)
            assert (before, after) == (w_before, w_after), (name, mcv, rate, which, seed)
            assert got.dtype == np.uint64 and got.shape == want.shape and (got == want).all(), (name, mcv, rate, which, seed)


@pytest.mark.gpu
def test_gpu_stage_entry_refuses_what_breaks_its_bounds():
    from ratatosk_amd import api
    for ev, n_u, bins in (([(1 << 32) | 4, 3], 2, [0, 0]), ([5, 5], 1, [0]), ([(2 << 32) | 1], 2, [0, 0]), ([1], 1, [20])):
        with pytest.raises(api.RtkError):
            api.index_subsample_events(ev, n_u, bins, [1] * n_u, [1] * 20, 2, 0.5)
    with pytest.raises(api.RtkError):
        api.index_subsample_events([1], 1, [0], [1], [1] * 20, 65, 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("name", sorted(SETS))
def test_gpu_tool_writes_the_files_of_the_host_route(reads, tmp_path, name, k):
    tmp, sr = str(tmp_path), reads[name]
    a = _build(sr, os.path.join(tmp, "fast"), k, ["--fast", "--subsample-colours"])
    b = _build(sr, os.path.join(tmp, "gpu"), k, ["--gpu", "--subsample-colours"])
    _assert_subsampled(_line(a[2]))
    assert "rtk_index_colour:" in b[2] and "left after subsampling" in b[2] and "colours on the host threads" not in b[2], b[2]  # the device thinned the events
    assert _line(a[2]) == _line(b[2])
    assert a[0] == b[0] and a[1] == b[1]
    c = _build(sr, os.path.join(tmp, "gpu_host"), k, ["--gpu", "--subsample-colours"], env={"RTK_INDEX_HOST_COLOURS": "1"})  # the host step on events of the host threads
    assert "left after subsampling" not in c[2] and a[1] == c[1]


@pytest.mark.gpu
def test_gpu_tool_with_colour_reads(tmp_path, monkeypatch):
    tmp = str(tmp_path)
    pre = _simulate(tmp, "cr", SETS["het_repeats"], lr=("--lr-n", "400", "--lr-len", "3000", "--lr-err", "0.01"))
    sr, lr = pre + ".sr.fq", pre + ".lr.fq"
    monkeypatch.setenv("RTK_INDEX_THREADS", "16")
    for k in (31, 63):  # second-pass index: every long read its own id
        a = _build(sr, os.path.join(tmp, "cr_fast"), k, ["--fast", "--subsample-colours", "--colour-reads", lr])
        b = _build(sr, os.path.join(tmp, "cr_gpu"), k, ["--gpu", "--subsample-colours", "--colour-reads", lr])
        _assert_subsampled(_line(a[2]))
        assert a[0] == b[0] and a[1] == b[1] and _line(a[2]) == _line(b[2])


@pytest.mark.gpu
def test_gpu_tool_with_a_small_event_buffer(tmp_path, monkeypatch):
    """the small event buffer of tests/test_index_build.py test_gpu_index_colours_with_a_small_event_buffer, on its set: sorted and thinned out while the reads still come"""
    tmp = str(tmp_path)
    monkeypatch.setenv("RTK_INDEX_THREADS", "16")
    sr = _simulate(tmp, "ev", ["--seed", "11", "--ref-len", "30000", "--het", "0.004", "--repeat-frac", "0.1", "--sr-cov", "40", "--sr-err", "0.01"]) + ".sr.fq"
    a = _build(sr, os.path.join(tmp, "ev_fast"), 31, ["--fast", "--subsample-colours"])
    _assert_subsampled(_line(a[2]))
    b = _build(sr, os.path.join(tmp, "ev_gpu0"), 31, ["--gpu", "--subsample-colours"])
    n_distinct = int(re.search(r"-> (\d+) distinct", b[2]).group(1))
    assert n_distinct == _line(a[2])["events"][0]
    monkeypatch.setenv("RTK_INDEX_EVENTS", str(n_distinct * 3 // 2))
    b = _build(sr, os.path.join(tmp, "ev_gpu"), 31, ["--gpu", "--subsample-colours"])
    assert int(re.search(r"thinned out (\d+) times", b[2]).group(1)) >= 1, b[2]
    assert a[0] == b[0] and a[1] == b[1]


@pytest.mark.gpu
def test_gpu_job_entries_over_several_sort_and_unique_rounds(reads, tmp_path, monkeypatch, capfd):
    """rtk_index_colour_cov and rtk_index_colour_end_subsampled through the C ABI, the reads fed in eight chunks into an event buffer of twice the distinct events:
    the buffer is sorted and thinned out several times before the end (the tool feeds a small input as one chunk per thread, so how often is up to its threads;
    here it is fixed). Coverage and thinned events equal those of a job with the default buffer, ended by rtk_index_colour_end and thinned by the stage entry."""
    import ctypes as C
    from ratatosk_amd import api
    from oracle import oracle_py as op
    tmp, sr, k = str(tmp_path), reads["het_repeats"], 31
    base = os.path.join(tmp, "base")
    _build(sr, base, k, ["--fast"])
    seqs = [l for l in gzip.open(base + ".index.k31.fasta.gz", "rt").read().split("\n") if l and l[0] != ">"]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(s) for s in seqs])
    pool = "".join(seqs).encode()
    rd = [r[1] for r in op.read_fastq(sr)]
    L = api.load_library()
    u64p, u32p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_ubyte)
    L.rtk_index_colour_begin.argtypes = [C.c_int, C.c_int, C.c_char_p, u64p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.rtk_index_colour_chunk.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, u64p, u32p, C.c_uint32]
    L.rtk_index_colour_end.argtypes = [C.c_void_p, C.POINTER(u64p), u64p, C.POINTER(u64p)]

    def ok(rc):
        assert rc == 0, L.rtk_last_error().decode()

    def feed(n_chunks):
        job = C.c_void_p()
        ok(L.rtk_index_colour_begin(0, k, pool, off.ctypes.data_as(u64p), len(seqs), C.byref(job)))
        per = (len(rd) + n_chunks - 1) // n_chunks
        for c in range(0, len(rd), per):
            part = rd[c:c + per]
            chars = ("\n".join(part) + "\n").encode()
            starts = np.zeros(len(part), dtype=np.uint64); starts[1:] = np.cumsum([len(s) + 1 for s in part[:-1]])
            ids = np.array([(c + i) // 2 for i in range(len(part))], dtype=np.uint32)  # a pair keeps one id
            ok(L.rtk_index_colour_chunk(job, chars, len(chars), starts.ctypes.data_as(u64p), ids.ctypes.data_as(u32p), len(part)))
        return job

    def take(p, n):
        a = np.ctypeslib.as_array(p, shape=(max(1, n),))[:n].copy()
        L.rtk_free(p)
        return a

    monkeypatch.setenv("RTK_INDEX_TRACE", "1")
    job = feed(1)
    ev_p, cov_p, n_ev = u64p(), u64p(), C.c_uint64()
    ok(L.rtk_index_colour_end(job, C.byref(ev_p), C.byref(n_ev), C.byref(cov_p)))
    events, cov = take(ev_p, n_ev.value), take(cov_p, len(seqs))
    assert n_ev.value > 10000
    rnd = random.Random(3)
    bin_of = np.array([rnd.choice(list(range(20)) + [255]) for _ in seqs], dtype=np.uint8)
    forced = np.array([rnd.randrange(3) != 0 for _ in seqs], dtype=np.uint8)
    sampled = np.array([j % 4 != 0 for j in range(20)], dtype=np.uint8)
    want, w_before, w_after = api.index_subsample_events(events, len(seqs), bin_of, forced, sampled, MCV, 0.3, seed=9)
    assert 0 < len(want) < len(events) and w_after < w_before
    capfd.readouterr()
    monkeypatch.setenv("RTK_INDEX_EVENTS", str(2 * n_ev.value))
    job = feed(8)
    ok(L.rtk_index_colour_cov(job, C.byref(cov_p)))
    assert (take(cov_p, len(seqs)) == cov).all()
    n_before, before, after = C.c_uint64(), C.c_uint64(), C.c_uint64()
    ok(L.rtk_index_colour_end_subsampled(job, bin_of.ctypes.data_as(u8p), forced.ctypes.data_as(u8p), sampled.ctypes.data_as(u8p), 20, MCV, 0.3, 9,
                                         C.byref(ev_p), C.byref(n_ev), C.byref(n_before), C.byref(before), C.byref(after)))
    got = take(ev_p, n_ev.value)
    assert (n_before.value, before.value, after.value) == (len(events), w_before, w_after)
    assert got.shape == want.shape and (got == want).all()
    rounds = re.search(r"thinned out (\d+) times", capfd.readouterr().err)
    assert rounds and int(rounds.group(1)) >= 2, "one round only"


@pytest.mark.gpu
def test_gpu_one_command_with_subsampled_colours(tmp_path):
    """`Ratatosk correct -s ... --subsample-colours` on the device against the oracle's two passes on the index files of the subsampled HOST build: the correction
    path on ids that were renumbered. Both index steps receive the option; the run ends with OUT.fastq alone."""
    from oracle import oracle_py as op
    tmp = str(tmp_path)
    pre = _simulate(tmp, "both", ["--seed", "17", "--ref-len", "30000", "--het", "0.003", "--repeat-frac", "0.05", "--sr-cov", "60", "--sr-err", "0.002"], lr=("--lr-n", "40", "--lr-len", "3000", "--lr-err", "0.08"))
    sr, lr = pre + ".sr.fq", pre + ".lr.fq"
    raw = op.read_fastq(lr)
    # the oracle's passes on the host build's files
    a = _build(sr, os.path.join(tmp, "h1"), 31, ["--fast", "--subsample-colours"])
    _assert_subsampled(_line(a[2]))
    g1 = op.Graph(os.path.join(tmp, "h1.index.k31.fasta.gz"), os.path.join(tmp, "h1.index.k31.rtsk"), 31)
    p1, _ = g1.correct_batch([r[1] for r in raw], [r[2] for r in raw], threads=8)
    mid = os.path.join(tmp, "h.2.fastq")
    with open(mid, "w") as f:
        for r, (s, q) in zip(raw, p1):
            f.write("@%s\n%s\n+\n%s\n" % (r[0], s, q))
    _build(sr, os.path.join(tmp, "h2"), 63, ["--fast", "--subsample-colours", "--colour-reads", mid])
    g2 = op.Graph(os.path.join(tmp, "h2.index.k63.fasta.gz"), os.path.join(tmp, "h2.index.k63.rtsk"), 63)
    want = g2.correct_batch2([s for s, _ in p1], [q for _, q in p1], [r[1] for r in raw], g2.opts(long_read_correct=1), threads=8)
    # one command on the device
    sub = os.path.join(tmp, "one"); os.mkdir(sub)
    out = os.path.join(sub, "out")
    r = subprocess.run([EXE, "correct", "-v", "-c", "2", "-s", sr, "--subsample-colours", "-l", lr, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    steps = [l for l in r.stderr.splitlines() if "rtk_build_index)" in l and ("step 1" in l or "step 3" in l)]
    assert len(steps) == 2 and all("--subsample-colours" in l and "--gpu" in l for l in steps), r.stderr
    _assert_subsampled(_line(r.stderr))  # (the first index step's line)
    assert r.stderr.count("rtk_build_index: subsample:") == 2
    got = op.read_fastq(out + ".fastq")
    assert [g[0] for g in got] == [x[0] for x in raw]
    assert [(g[1], g[2]) for g in got] == want
    assert sum(1 for (s, _), x in zip(want, raw) if s != x[1]) > 0
    assert sorted(os.listdir(sub)) == ["out.fastq"], os.listdir(sub)
