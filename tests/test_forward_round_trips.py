"""The forward strand of a gap region does not walk an alignment that nobody reads (csrc/hip/rtk_region_align.h, rtk_trim_by_column and rtk_park_walk).

The forward trim of a gap region stores its NW sweep, which also holds the alignment the consensus would ask for. Since most gap regions skip their second strand
and with it the consensus (§3.2 (f)), the trim keeps only what the rule of the skip reads -- that the alignment exists, its distance, its last move -- and the
region program walks the path and parks it where the second strand does run. RTK_PARK_EAGER=1 walks at the trim, as before.

Checked per set (the 1 Mb set and the hard genomes `all` and `microsatellite` of tests/test_second_strand.py at k = 31 and 21, the pass-2 set of tests/test_pass2.py),
on the 1-lane simulator and on the MI355X, under the default, RTK_PARK_EAGER=1, RTK_STRAND2_ALWAYS=1, RTK_STRAND2_AUDIT=1 and the default with the other reading
of [A3] (tests/test_a3_switch.py): the corrected reads equal the oracle's; the second-strand counters relate as tests/test_second_strand.py finds them and do not
depend on when the walk is made; every stored sweep is either walked or never walked (n_park_walked + n_park_deferred == n_trim_stored), a walk is made only for
a region that runs its second strand, and some still are. On the 1 Mb set at least 90 % of the stored sweeps are never walked (10 419 of 10 480 on the
simulator) and the walks that remain make at most 0.65 of the moves of RTK_PARK_EAGER=1 (4 736 106 moves there, of which about 2.06 M belong to the parked
paths: 0.57 expected; the margin is for the 61 regions that keep both strands). The GPU tier also holds the work counters of the wave kernels (n_expand,
n_colour_elem, n_align, n_align_cells, the moves and the walks) to those of the simulator, set by set: both builds take the same alignment routes, the stored
sweep that scores a terminal candidate and serves its quality string (rtk_myers_nw_and_save, csrc/hip/rtk_myers_align.h) included."""
import pytest

import test_pass2 as P2
import test_second_strand as S2
from conftest import SIM_LIB
from oracle import oracle_py as op
from ratatosk_amd import api

EAGER, A3 = "RTK_PARK_EAGER", "RTK_A3_ORDER"
SETTINGS = {"default": {}, "eager": {EAGER: "1"}, "always": {S2.ALWAYS: "1"}, "audit": {S2.AUDIT: "1"}, "a3": {A3: "strand"}}
SETS = ["one_mb", "all-k31", "all-k21", "microsatellite-k31", "microsatellite-k21", "pass2"]
WORK = ("n_expand", "n_colour_elem", "n_align", "n_align_cells")
_cache = {}


def _env(monkeypatch, setting):
    for knob in (EAGER, S2.ALWAYS, S2.AUDIT, A3):
        monkeypatch.delenv(knob, raising=False)
    for knob, v in SETTINGS[setting].items():
        monkeypatch.setenv(knob, v)  # read on every call (rtk_knobs.h); [A3] when the options are made


def _case(name, tmp_factory, monkeypatch):
    """the set, its reads and the oracle's bytes under both readings of [A3]: made once per session"""
    if name in _cache:
        return _cache[name]
    tmp = tmp_factory.mktemp("frt_" + name.replace("-", "_"))
    c = {"name": name, "k": 31, "raws": None, "p2": name == "pass2", "sim": {}}
    if name == "pass2":
        c["pre"] = P2._second_pass_set(tmp, "p2", ["--seed", 31, "--ref-len", 40000, "--het", 0.004, "--repeat-frac", 0.05, "--sr-cov", 40, "--sr-err", 0.005,
                                                   "--lr-n", 60, "--lr-len", 3000, "--lr-profile", "ont", "--lr-err", 0.08])
        og, _, c["seqs"], c["quals"], c["raws"] = P2._load(c["pre"], SIM_LIB)
    else:
        if name == "one_mb":
            c["pre"] = S2._one_mb_set(tmp)
        else:
            kind, k = name.split("-k")
            c["k"] = int(k)
            c["pre"] = S2._hard_set(tmp, kind, c["k"])
        reads = op.read_fastq(c["pre"] + ".lr.fq")
        c["seqs"], c["quals"] = [r[1] for r in reads], [r[2] for r in reads]
        og = op.Graph(c["pre"] + ".index.k%d.fasta.gz" % c["k"], c["pre"] + ".index.k%d.rtsk" % c["k"], c["k"])
    c["want"] = {}
    for reading in ("default", "a3"):
        _env(monkeypatch, reading)
        if c["p2"]:
            c["want"][reading] = [(w[0], w[1]) for w in og.correct_batch2(c["seqs"], c["quals"], c["raws"], og.opts(long_read_correct=1), threads=8)]
        else:
            c["want"][reading] = og.correct_batch(c["seqs"], c["quals"], threads=8)[0]
    _env(monkeypatch, "default")
    _cache[name] = c
    return c


def _graph(c, lib):
    if c["p2"]:
        return P2._load(c["pre"], lib)[1]
    return api.Graph(c["pre"] + ".index.k%d.fasta.gz" % c["k"], c["pre"] + ".index.k%d.rtsk" % c["k"], c["k"], device=0, lib_path=lib)


def _sim_default(c, monkeypatch):
    """the simulator's run under the default: once per set"""
    if "default" not in c["sim"]:
        c["sim"]["default"] = _run(c, _graph(c, SIM_LIB), "default", monkeypatch)
    return c["sim"]["default"]


def _run(c, pg, setting, monkeypatch):
    _env(monkeypatch, setting)
    b = api.Batch(pg, c["seqs"], c["quals"], raw=c["raws"]) if c["p2"] else api.Batch(pg, c["seqs"], c["quals"])
    b.run(pg.opts(long_read_correct=1) if c["p2"] else pg.opts())
    got, st = b.fetch(), b.stats()
    _env(monkeypatch, "default")
    got = [(g[0], g[1]) for g in got] if c["p2"] else got
    want = c["want"]["a3" if setting == "a3" else "default"]
    assert got == want, "%s, %s: %d reads differ from the oracle" % (c["name"], setting, sum(1 for a, b_ in zip(got, want) if a != b_))
    return st


def _check(name, lib, tmp_factory, monkeypatch):
    c = _case(name, tmp_factory, monkeypatch)
    pg = _graph(c, lib)
    st = {setting: (_sim_default(c, monkeypatch) if lib is not None and setting == "default" else _run(c, pg, setting, monkeypatch)) for setting in SETTINGS}
    for setting, x in st.items():
        print("%s %s: second strands run %d skipped %d mismatches %d; sweeps stored %d walked %d never walked %d; moves %d; n_expand %d n_colour_elem %d n_align %d n_align_cells %d" % (
            name, setting, x["n_strand2_run"], x["n_strand2_skipped"], x["n_strand2_audit_mismatch"], x["n_trim_stored"], x["n_park_walked"], x["n_park_deferred"], x["n_moves"],
            x["n_expand"], x["n_colour_elem"], x["n_align"], x["n_align_cells"]))
    d, e, al, au = st["default"], st["eager"], st["always"], st["audit"]
    # the second strand, as tests/test_second_strand.py finds it -- and the same whenever the walk is made
    assert S2._counts(e) == S2._counts(d) == S2._counts(au)
    assert d["n_strand2_run"] + d["n_strand2_skipped"] == al["n_strand2_run"] + al["n_strand2_skipped"] and al["n_strand2_skipped"] == 0
    assert all(x["n_strand2_audit_mismatch"] == 0 for x in st.values())
    assert d["n_strand2_run"] > 0
    # every stored sweep is walked or left alone; a walk belongs to a region that runs its second strand (a region its forward strand settles has no trim)
    for x in st.values():
        assert x["n_park_walked"] + x["n_park_deferred"] == x["n_trim_stored"]
    for x in (d, st["a3"]):
        assert 0 < x["n_park_walked"] <= x["n_strand2_run"]
    assert al["n_park_walked"] <= al["n_strand2_run"] and au["n_park_walked"] <= au["n_strand2_run"] + au["n_strand2_skipped"]
    assert e["n_park_walked"] >= d["n_park_walked"] and e["n_moves"] >= d["n_moves"]
    assert e["n_park_walked"] == al["n_park_walked"] == au["n_park_walked"]  # every sweep that can be parked, whichever way it comes to its walk
    for w in WORK + ("n_trim_stored", "n_consensus_resumed", "n_consensus_swept"):
        assert e[w] == d[w], w  # the deferral moves a walk, nothing else
    if name == "one_mb":
        assert d["n_park_deferred"] >= 0.9 * d["n_trim_stored"], (d["n_park_deferred"], d["n_trim_stored"])
        assert d["n_moves"] <= 0.65 * e["n_moves"], (d["n_moves"], e["n_moves"])
    if lib is None:  # the wave kernels do the work the 1-lane simulator does
        sim = _sim_default(c, monkeypatch)
        for w in WORK + ("n_park_walked", "n_park_deferred", "n_moves"):
            assert d[w] == sim[w], (w, d[w], sim[w])
    return d


# ---------------------------------------------------------------------------------------------------------------------------------- simulator tier
@pytest.mark.parametrize("name", SETS)
def test_sim_forward_round_trips(tmp_path_factory, monkeypatch, name):
    _check(name, SIM_LIB, tmp_path_factory, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_gpu_forward_round_trips(tmp_path_factory, monkeypatch, name):
    _check(name, None, tmp_path_factory, monkeypatch)



@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_gpu_alignment_counters_equal_simulator(tmp_path_factory, monkeypatch, name):
    """n_align and n_align_cells of the wave kernels equal the 1-lane simulator's: the simulator build takes the stored-sweep route of rtk_myers_nw_and_save too
    (1 Mb set, default: 48 410 alignments, 24 485 310 word-columns in both builds; without that route the simulator made 66 470 and 26 888 198)."""
    c = _case(name, tmp_path_factory, monkeypatch)
    d, sim = _run(c, _graph(c, None), "default", monkeypatch), _sim_default(c, monkeypatch)
    print("%s: n_align %d (simulator %d), n_align_cells %d (simulator %d)" % (name, d["n_align"], sim["n_align"], d["n_align_cells"], sim["n_align_cells"]))
    assert (d["n_align"], d["n_align_cells"]) == (sim["n_align"], sim["n_align_cells"])
