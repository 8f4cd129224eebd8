"""The forward trim of a gap region stores no table: its sweep keeps the delta vectors of the LAST column, and the last move of the alignment it parks is derived
from them (csrc/hip/rtk_myers_sweep.h, rtk_myers_fast32 / rtk_myers_fast with STORE = 2; rtk_myers_walk.h, rtk_myers_last_move_column; csrc/hip/rtk_region_align.h).

Cell (keep, |raw|) of the sweep of (corrected, raw): the vertical delta is bit keep - 1 of Pv / Mv of the last column, the horizontal delta the same bit of Ph / Mh,
and the diagonal neighbour lies one horizontal delta -- that of row keep - 1: the bit before, in the word before at a word boundary, +1 in row 0 -- to the left of the
cell above. The stage entry rtk_myers_batch holds that derivation (test-only mode 6) to the look at a stored table (mode 5, tests/test_park_last_move.py) and to the
walk itself (mode 4, tests/test_trim_column.py):

* every NW path row of the reference's golden vectors: the last operation of its cigar;
* seeded random pairs with queries of 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049 characters (the sweep works on 32-bit words up to 2048 characters and on 64-bit
  words beyond) and 4096 (the cap of the route) against targets of 1, 63, 64, 65 and 200, at the rows 1, every multiple of 32 with its two neighbours, and |q|;
  the targets are noisy copies of a stretch of the query, cut so that paths end in inserts, deletes, matches and mismatches, and every move must turn up as a
  last one. A cigar does not tell a match from a mismatch: for strings of A C G T the last move is a match exactly when the two last characters are equal.

Each call counts the problems the route took (rtk_myers_column_last_routes): the same under modes 5 and 6. On the 1-lane simulator a sweep of mode 6 leaves the
last column's entries and overwrites the rest of the table, so a read of anything else shows."""
import random

import pytest

import test_park_last_move as PL
import test_trim_column as TC
from conftest import SIM_LIB, golden_rows
from ratatosk_amd import api

Q_LENS = (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4096)
T_LENS = (1, 63, 64, 65, 200)


def _last(lib, mode, qs, ks, ts):
    """[(distance, last move or None)] of mode 5 or 6, with the route count checked"""
    res = api.myers_batch(qs, ts, ks, [mode] * len(qs), want_path=False, lib_path=lib)
    col, fb = api.myers_column_last_routes(lib)
    must = sum(1 for q, k, t in zip(qs, ks, ts) if TC._prefix_takes_column(q, k, t))
    assert (col, fb) == (must, len(qs) - must), (mode, col, fb, must)
    out = []
    for d, locs, _ in res:
        assert len(locs) == 1
        out.append((d, None if locs[0] < 0 else locs[0]))
    return out


def _rows(m):
    """row 1, every word boundary of the 32-bit and the 64-bit sweep with its two neighbours, and row m"""
    ks = {1, m}
    for b in range(32, m + 2, 32):
        ks |= {b - 1, b, b + 1}
    return sorted(k for k in ks if 1 <= k <= m)


def _problems(seed):
    rnd = random.Random(seed)
    s = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    noisy = lambda x: "".join(c if rnd.random() > 0.1 else rnd.choice(("", rnd.choice("ACGT"), c + rnd.choice("ACGT"))) for c in x)
    out = []
    for m in Q_LENS:
        q = s(m)
        for n in T_LENS:
            rows = _rows(m)
            # four targets per shape: a copy of the query's start (rows beyond it end in inserts, rows before it in deletes), a copy of the stretch that ends at a
            # row (match or mismatch at that row), unrelated characters, and the first with another last character
            a = (noisy(q[:n]) + s(n))[:n]
            at = rows[len(rows) // 2]
            b = (s(n) + noisy(q[max(0, at - n):at]))[-n:]
            c = s(n)
            d = a[:-1] + ("A" if a[-1] != "A" else "C")
            for t in (a, b, c, d):
                assert len(t) == n
                out.extend((q, k, t) for k in rows)
    # what the route leaves to the calls it replaces: a target byte the sweep cannot hold, row 0
    out.append((s(100), 64, s(30) + "N" + s(30)))
    out.append((s(100), 0, s(50)))
    return out


def _golden(lib):
    rnd = random.Random(5)
    rows = [r for r in golden_rows() if r["mode"] == 0 and r["path"] and r["d"] >= 0]
    qs = [r["q"] + "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(1, 200))) for r in rows]
    ks, ts = [len(r["q"]) for r in rows], [r["t"] for r in rows]
    got = _last(lib, api.MODE_NW_PREFIX_LAST_COLUMN, qs, ks, ts)
    assert got == _last(lib, api.MODE_NW_PREFIX_LAST, qs, ks, ts)
    seen = set()
    for r, q, k, t, g in zip(rows, qs, ks, ts, got):
        mv = PL._check(q, k, t, r["d"], r["cigar"], g)
        if TC._prefix_takes_column(q, k, t):
            seen.add(mv)
    assert {1, 2} <= seen and (0 in seen or 3 in seen), seen


def _random(lib, seed):
    probs = _problems(seed)
    qs, ks, ts = [p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs]
    col = _last(lib, api.MODE_NW_PREFIX_LAST_COLUMN, qs, ks, ts)
    tab = _last(lib, api.MODE_NW_PREFIX_LAST, qs, ks, ts)
    bad = [(len(q), k, len(t), c, x) for q, k, t, c, x in zip(qs, ks, ts, col, tab) if c != x]
    assert not bad, (len(bad), bad[:5])  # the last column against the stored table
    # mode 4, the walk itself: every row of the short queries; of the long ones row 1, the first two word boundaries, the boundary at 2048 and the last one, each
    # with its neighbours, and row |q| (a walk returns a path of up to |q| + |t| moves per problem; mode 5 above covers every row, and
    # tests/test_park_last_move.py holds mode 5 to the walk)
    def walked_too(m, k):
        return m <= 65 or k <= 2 or k >= m - 1 or any(abs(k - b) <= 1 for b in (32, 64, 2048, (m - 1) // 64 * 64))
    pick = [i for i, (q, k, t) in enumerate(probs) if walked_too(len(q), k)]
    qs, ks, ts, col = [qs[i] for i in pick], [ks[i] for i in pick], [ts[i] for i in pick], [col[i] for i in pick]
    walked = []
    for i in range(0, len(qs), 256):
        walked += api.myers_batch(qs[i:i + 256], ts[i:i + 256], ks[i:i + 256], [api.MODE_NW_PREFIX] * len(qs[i:i + 256]), want_path=True, lib_path=lib)
    seen, by_shape = {}, {}
    for q, k, t, (d, _, cig), g in zip(qs, ks, ts, walked, col):
        mv = PL._check(q, k, t, d, cig, g)
        if TC._prefix_takes_column(q, k, t):
            seen[mv] = seen.get(mv, 0) + 1
            by_shape.setdefault((len(q), len(t)), set()).add(mv)
    print("last moves by kind:", sorted(seen.items()))
    assert all(seen.get(mv, 0) > 0 for mv in (0, 1, 2, 3)), seen  # insert, delete, match and mismatch all end a path
    assert set(by_shape) == {(m, n) for m in Q_LENS for n in T_LENS}  # every shape took the route


# ---------------------------------------------------------------------------------------------------------------------------------- simulator tier
def test_sim_last_column_move_golden():
    _golden(SIM_LIB)


def test_sim_last_column_move_random():
    _random(SIM_LIB, 41)


# ---------------------------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_gpu_last_column_move_golden():
    _golden(None)


@pytest.mark.gpu
def test_gpu_last_column_move_random():
    _random(None, 42)
