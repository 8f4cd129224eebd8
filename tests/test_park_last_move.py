"""The forward trim of a gap region keeps the LAST move of the alignment it parks, not the path (csrc/hip/rtk_myers_walk.h, rtk_myers_last_move; csrc/hip/rtk_region_align.h,
rtk_trim_by_column and rtk_park_walk).

The rule that skips the second strand of a gap region asks of the parked alignment NW(corrected[0, keep), raw) only that it exists, its distance and whether its
last move is an insert. The path is walked backwards from cell (keep, |raw|) of the stored sweep, so its last move is the walk's first step: one look at the table.
The stage entry rtk_myers_batch holds that look to the walk itself through the test-only mode 5 (distance and last move of the NW path of query[0, k), read off
the stored sweep of the whole query without a walk) next to mode 4 (the same path, walked; tests/test_trim_column.py):

* every NW path row of the reference's golden vectors: the last operation of its cigar;
* seeded random pairs of 1 - 200 characters at the prefix rows 1, 63, 64, 65, 127, 128, 129 and |q| (the word boundaries of the table), built to end in each
  move -- a query that runs on past the target ends in an insert, a target that runs on in a delete, an equal tail in a match --, against mode 4 on the same
  problems. A cigar does not tell a match from a mismatch: for strings of A C G T the last move is a match exactly when the two last characters are equal.

Each check counts the problems the route took (rtk_myers_column_last_routes): exactly those that _prefix_takes_column of tests/test_trim_column.py lets through;
the others are answered from the path of the call the route replaces. The 1-lane simulator and the wave kernels read the same table entries."""
import random

import pytest

import test_trim_column as TC
from conftest import SIM_LIB, golden_rows
from ratatosk_amd import api

ROWS = (1, 63, 64, 65, 127, 128, 129)
OPS = {0: "M", 1: "I", 2: "D", 3: "M"}


def _last_moves(lib, qs, ks, ts):
    """[(distance, last move or None)] of mode 5, with the route count checked"""
    res = api.myers_batch(qs, ts, ks, [api.MODE_NW_PREFIX_LAST] * len(qs), want_path=False, lib_path=lib)
    col, fb = api.myers_column_last_routes(lib)
    must = sum(1 for q, k, t in zip(qs, ks, ts) if TC._prefix_takes_column(q, k, t))
    assert (col, fb) == (must, len(qs) - must)
    out = []
    for d, locs, _ in res:
        assert len(locs) == 1
        out.append((d, None if locs[0] < 0 else locs[0]))
    return out, col, fb


def _check(q, k, t, d, cigar, got):
    gd, mv = got
    assert gd == d, (q[:k], t, gd, d)
    if not cigar:
        assert mv is None, (q[:k], t, mv)
        return None
    assert mv in OPS and OPS[mv] == cigar[-1], (q[:k], t, mv, cigar)
    if mv in (0, 3) and TC._acgt(q[:k]) and TC._acgt(t):
        assert (mv == 0) == (q[k - 1] == t[-1]), (q[:k], t, mv)
    return mv


def _golden(lib):
    rnd = random.Random(5)
    rows = [r for r in golden_rows() if r["mode"] == 0 and r["path"] and r["d"] >= 0]
    qs = [r["q"] + "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(1, 200))) for r in rows]
    ks, ts = [len(r["q"]) for r in rows], [r["t"] for r in rows]
    got, col, fb = _last_moves(lib, qs, ks, ts)
    seen = set()
    for r, q, k, t, g in zip(rows, qs, ks, ts, got):
        mv = _check(q, k, t, r["d"], r["cigar"], g)
        if TC._prefix_takes_column(q, k, t):
            seen.add(mv)
    assert col > 0 and {1, 2} <= seen and (0 in seen or 3 in seen), (col, seen)


def _pairs(seed, n):
    """(query, prefix row, target): the target is the query's prefix with edits, then a tail that decides the last move"""
    rnd = random.Random(seed)
    s = lambda m: "".join(rnd.choice("ACGT") for _ in range(m))
    out = []
    for i in range(n):
        base = s(rnd.randrange(1, 201))
        t = "".join(c if rnd.random() > 0.08 else rnd.choice(("", rnd.choice("ACGT"), c + rnd.choice("ACGT"))) for c in base) or "A"
        kind = i % 4
        if kind == 0:
            q = base + s(rnd.randrange(1, 12))          # the query runs on: the path ends in inserts
        elif kind == 1:
            q, t = base, t + s(rnd.randrange(1, 12))    # the target runs on: deletes
        elif kind == 2:
            tail = s(rnd.randrange(1, 12)); q, t = base + tail, t + tail  # an equal tail: a match
        else:
            q, t = base + "A", t + "C"                  # two different last characters
        q, t = q[:200], t[:200]
        if i % 23 == 0:
            t = t[:len(t) // 2] + "N" + t[len(t) // 2 + 1:]  # a target byte the sweep cannot hold: the fallback answers
        for k in sorted(set(r for r in ROWS if r <= len(q)) | {len(q)}):
            out.append((q, k, t))
        if i % 31 == 0:
            out.append((q, 0, t))  # row 0: no path
        out.append((q + s(rnd.randrange(1, 150)), len(q), t))  # the trim's case: the swept string runs on past the row
    return out


def _random(lib, seed, n):
    probs = _pairs(seed, n)
    qs, ks, ts = [p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs]
    walked = api.myers_batch(qs, ts, ks, [api.MODE_NW_PREFIX] * len(qs), want_path=True, lib_path=lib)  # mode 4: the walk itself
    got, col, fb = _last_moves(lib, qs, ks, ts)
    seen = {}
    for q, k, t, (d, _, cig), g in zip(qs, ks, ts, walked, got):
        mv = _check(q, k, t, d, cig, g)
        if TC._prefix_takes_column(q, k, t):
            seen[mv] = seen.get(mv, 0) + 1
    assert col > 0 and fb > 0
    assert all(seen.get(mv, 0) > 0 for mv in (0, 1, 2, 3)), seen  # the route met every move as a last one
    return seen


# ---------------------------------------------------------------------------------------------------------------------------------- simulator tier
def test_sim_last_move_golden():
    _golden(SIM_LIB)


def test_sim_last_move_random_vs_walk():
    _random(SIM_LIB, 21, 60)


# ---------------------------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_gpu_last_move_golden():
    _golden(None)


@pytest.mark.gpu
def test_gpu_last_move_random_vs_walk():
    _random(None, 22, 150)
