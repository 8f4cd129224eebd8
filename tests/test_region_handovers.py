"""The forward trim of a gap region stores no table (csrc/hip/rtk_region_align.h, rtk_trim_by_column and rtk_park_walk).

The forward trim keeps the last column of its sweep instead of the table, and a region that walks the alignment after all sweeps the pair a second time
(RTK_TRIM_STORE=1: the table at the trim, no second sweep).

Per set (those of tests/test_forward_round_trips.py: the 1 Mb set, the hard genomes at k = 31 and 21, the pass-2 set) and per setting -- the default, the knob, and
RTK_STRAND2_ALWAYS=1, RTK_STRAND2_AUDIT=1, RTK_PARK_EAGER=1 with and without the knob -- the corrected reads equal the oracle's, the work counters n_expand,
n_colour_elem, n_path_base, n_moves, n_align and n_align_cells of the old route equal the new route's, no audit finds a mismatch, and
n_park_resweeps == n_park_walked wherever no table is kept (0 second sweeps with RTK_TRIM_STORE=1). Every set holds head or tail regions (trims without a stored
sweep beyond those of the second strands). One run of the 1 Mb set has min_score > 0, another route through the path search that ends in the same trim. The GPU
tier runs the 1 Mb set and one hard genome and holds the counters to the simulator's."""
import pytest

import test_forward_round_trips as FR
from conftest import SIM_LIB

KNOBS = ("RTK_TRIM_STORE",)
WORK = ("n_expand", "n_colour_elem", "n_path_base", "n_moves", "n_align", "n_align_cells", "n_trim_stored", "n_park_walked", "n_park_deferred", "n_strand2_run", "n_strand2_skipped")
SETS = ["one_mb", "all-k31", "all-k21", "pass2"]
GPU_SETS = ["one_mb", "all-k31"]


def _run(c, pg, monkeypatch, knob=None, setting="default"):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if knob:
        monkeypatch.setenv(knob, "1")  # read on every call (rtk_knobs.h)
    try:
        return FR._run(c, pg, setting, monkeypatch)  # asserts the bytes against the oracle
    finally:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)


def _check(name, lib, tmp_factory, monkeypatch):
    c = FR._case(name, tmp_factory, monkeypatch)
    pg = FR._graph(c, lib)
    d = _run(c, pg, monkeypatch)
    print("%s default: %s resweeps %d" % (name, {w: d[w] for w in WORK}, d["n_park_resweeps"]))
    assert d["n_park_walked"] > 0 and d["n_park_resweeps"] == d["n_park_walked"]
    # head and tail regions are there: only they and the second strands trim without a stored sweep (one trim per correct call that is not settled by its end test)
    assert d["n_trim_column"] + d["n_trim_fallback"] > d["n_strand2_run"], (d["n_trim_column"], d["n_trim_fallback"], d["n_strand2_run"])
    for setting in ("default", "always", "audit", "eager"):
        x = d if setting == "default" else _run(c, pg, monkeypatch, setting=setting)
        assert x["n_strand2_audit_mismatch"] == 0 and x["n_park_resweeps"] == x["n_park_walked"] > 0, setting
        old = _run(c, pg, monkeypatch, knob="RTK_TRIM_STORE", setting=setting)
        for w in WORK:
            assert old[w] == x[w], (setting, w, old[w], x[w])
        assert old["n_park_resweeps"] == 0
    if lib is None:
        sim = _run(c, FR._graph(c, SIM_LIB), monkeypatch)
        for w in WORK + ("n_park_resweeps",):
            assert d[w] == sim[w], (w, d[w], sim[w])


def _check_min_score(lib, tmp_factory, monkeypatch):
    """min_score > 0: non-terminal sub-paths are scored where they are found (rtk_explore_subgraph, lazy_nt false); bytes against the oracle under both trim routes"""
    from oracle import oracle_py as op
    from ratatosk_amd import api
    c = FR._case("one_mb", tmp_factory, monkeypatch)
    og = op.Graph(c["pre"] + ".index.k31.fasta.gz", c["pre"] + ".index.k31.rtsk", 31)
    want = og.correct_batch(c["seqs"], c["quals"], opts=og.opts(min_score=0.5), threads=8)[0]
    pg = FR._graph(c, lib)
    st = {}
    for knob in (None,) + KNOBS:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        if knob:
            monkeypatch.setenv(knob, "1")
        b = api.Batch(pg, c["seqs"], c["quals"])
        b.run(pg.opts(min_score=0.5))
        got, st[knob] = b.fetch(), b.stats()
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        assert got == want, "min_score 0.5, %s: %d reads differ from the oracle" % (knob, sum(1 for a, b_ in zip(got, want) if a != b_))
    for w in WORK:
        assert st[None][w] == st["RTK_TRIM_STORE"][w], w
    lazy = _run(c, pg, monkeypatch)
    print("n_align with min_score 0.5: %d, with 0: %d" % (st[None]["n_align"], lazy["n_align"]))
    assert st[None]["n_align"] > lazy["n_align"]  # non-terminal candidates were scored that min_score 0 never scores


def test_sim_region_handovers_min_score(tmp_path_factory, monkeypatch):
    _check_min_score(SIM_LIB, tmp_path_factory, monkeypatch)


@pytest.mark.gpu
def test_gpu_region_handovers_min_score(tmp_path_factory, monkeypatch):
    _check_min_score(None, tmp_path_factory, monkeypatch)


@pytest.mark.parametrize("name", SETS)
def test_sim_region_handovers(tmp_path_factory, monkeypatch, name):
    _check(name, SIM_LIB, tmp_path_factory, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SETS)
def test_gpu_region_handovers(tmp_path_factory, monkeypatch, name):
    _check(name, None, tmp_path_factory, monkeypatch)
