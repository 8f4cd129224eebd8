"""End bookkeeping of the semi-global modes (rtk_shw_ends, csrc/hip/rtk_myers_distance.h) at every word and schedule edge of the query length.

edlib pads the query to whole 64-row blocks, so SHW and HW report target position -1, with score |query|, when |query| % 64 != 0
(edlib.cpp:658-692): alone when it beats every column, in front of the columns when it ties with them.  One function decides that for every route.  api.myers_batch reaches
two of them: the general tail of rtk_myers_distance (the batch always asks for the list of locations, so the register sweep's branch, `!locs_out`, is
not taken) and the stored sweep of rtk_myers_path (want_path).  The register sweep's branch and the saved sweep of rtk_myers_nw_and_save are reached
by the region program (test_forward_round_trips.py, test_gpu_correct.py, the hard genomes), SHW by column by test_trim_column.py.
Here api.myers_batch is held to oracle_py.myers -- distance, every end location, cigar -- on the simulator, on the device
and on the device's multi-wave kernel, for query lengths around the 32- and 64-bit word edges, the last length of the 32-bit sweep (2048) and the first
of two row blocks (4097).  Four targets per length: one that contains the query, one without a base in common with a poly-A query, a short one whose best
column score is |query| exactly, and the first with an N in it (not plain A/C/G/T: the generic pass).  NW is the control.  HW has no path on the device
(rtk_myers_batch refuses it), so the cigar is compared for SHW and NW."""
import functools
import random

import pytest

from conftest import SIM_LIB
from oracle import oracle_py as op
from ratatosk_amd import api

LENGTHS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 2047, 2048, 2049, 4095, 4096, 4097]
NW, SHW, HW = 0, 1, 2
RUNS = [(SHW, False), (HW, False), (NW, False), (SHW, True), (NW, True)]  # (mode, want_path)


@functools.lru_cache(maxsize=None)
def cases():
    """[(query, target)], four per length, in the order of LENGTHS"""
    rnd = random.Random(20261021)
    out = []
    for m in LENGTHS:
        q = "".join(rnd.choice("ACGT") for _ in range(m))
        holds = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(1, 150))) + q + "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(1, 150)))
        out.append((q, holds))
        out.append(("A" * m, "C" * (m + rnd.randrange(1, 300))))  # every column of the last row scores >= m, the first m of them m: -1 ties with them
        q3 = "".join(rnd.choice("ACG") for _ in range(m))
        out.append((q3, "T" * min(m, 5)))                         # best column score == m exactly: -1 and the real ends all count
        at = rnd.randrange(len(holds))
        out.append((q, holds[:at] + "N" + holds[at + 1:]))
    assert len(out) < 200 and all(len(t) <= len(q) + 300 and len(t) <= 4400 for q, t in out)
    return out


@functools.lru_cache(maxsize=None)
def expected():
    """{(mode, want_path): [oracle result per case]}, computed once for the three tiers"""
    return {(mode, path): [op.myers(q, t, -1, mode, path) for q, t in cases()] for mode, path in RUNS}


def check(**where):
    cs = cases()
    for (mode, path), want in expected().items():
        got = api.myers_batch([q for q, _ in cs], [t for _, t in cs], None, [mode] * len(cs), want_path=path, **where)
        for (q, t), (d, locs, cig), w in zip(cs, got, want):
            what = (len(q), len(t), mode, path)
            assert d == w[0], what
            assert locs == w[1], what
            if path:
                assert cig == w[2], what


def test_the_oracle_reports_location_minus_one_in_the_cases_built_for_it():
    cs, ex = cases(), expected()
    for i, m in enumerate(LENGTHS):
        mine = range(4 * i, 4 * i + 4)
        assert all(len(cs[c][0]) == m for c in mine)
        for mode in (SHW, HW):
            hit = [c for c in mine if -1 in ex[(mode, False)][c][1]]
            if m % 64 != 0:
                assert hit, (m, mode)
                assert any(len(ex[(mode, False)][c][1]) > 1 for c in hit), (m, mode)  # ... and ties with real ends in one of them
            else:
                assert not hit, (m, mode)
        assert all(ex[(NW, False)][c][1] == [len(cs[c][1]) - 1] for c in mine)


def test_ends_on_the_simulator():
    check(lib_path=SIM_LIB)


@pytest.mark.gpu
def test_ends_on_the_device():
    check()


@pytest.mark.gpu
def test_ends_on_the_device_with_eight_waves():
    check(waves=8)
