"""The wave set primitives of the region stage, run on their own and compared with plain Python (stage entry rtk_sets_batch, api.sets_batch).

The colour selection of the region program (csrc/hip/rtk_colours.h) is built on a handful of wave-cooperative primitives, each written once for
the 1-lane simulator and once for the device: rtk_set_filter / rtk_set_union / rtk_set_inter_count and rtk_sort_pairs (rtk_sets.h), the two radix sorts, and the
bit vectors rtk_bm_from_ids / rtk_bm_lowest / rtk_bm_count with their 8-lane forms (rtk_colours.h). The device versions switch between code paths by size: the
searched set is staged in LDS when nb <= 2048 and na >= 16, the bitonic network runs in LDS up to 512 pairs and blocked above, the radix sorts make one pass per
key byte (rtk_radix_sort_u32 an even number of them), the 8-lane prefix sums are DPP moves. Every problem below sits on or next to one of those edges. One
launch holds them all, one problem per wavefront; the references are Python sets, sorted() and integers, nothing from the library.

Set operations: sizes on both sides of the staging switch and of the 64-lane chunk, every pair of sizes with na * nb below 5 million, eight relations between
the two sets. INTER_COUNT may stop counting anywhere at or above its cap: the result must be the true count when that is below the cap, else at least the cap
(and never above the true count). SORT_PAIRS: a pair of two all-ones words cannot be told from the padding rtk_sort_pairs appends, so values stay below 2^63.
The radix sorts and the 8-lane vectors exist on the device only: the simulator answers those problems "not in this build", and the simulator test skips them
and nothing else."""
import functools

import numpy as np
import pytest

from conftest import SIM_LIB
from ratatosk_amd import api

SET_SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 5000)
SET_PRODUCT_LIMIT = 5_000_000
SORT_SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097)
RADIX_SIZES = (0, 1, 63, 64, 65, 256, 511, 512, 513, 1663, 1664)
RADIX_MAX_KEYS = (0, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 32) - 1)
UNIVERSES = (1, 63, 64, 65, 511, 512, 513, 1664, 4096)
DEVICE_ONLY = (api.SETS_RADIX_U32, api.SETS_RADIX_PAIRS_U32, api.SETS_BM8_LOWEST)
TOP = 0xFFFFFFFE


def _sorted_sample(r, n, lo, hi):
    """n distinct integers of [lo, hi), ascending"""
    s = set()
    while len(s) < n:
        s.update(r.randint(lo, hi, size=2 * (n - len(s)) + 8, dtype=np.int64).tolist())
    return sorted(r.permutation(sorted(s))[:n].tolist())


def _relations(r, na, nb):
    """(name, a, b) for every relation the two sizes allow"""
    out = [("disjoint", [3 * i + 10 for i in range(na)], [3 * j + 11 for j in range(nb)]),
           ("interleaved", [2 * i for i in range(na)], [3 * j for j in range(nb)]),
           ("a-below-b", [i + 5 for i in range(na)], [na + 100 + j for j in range(nb)]),
           ("b-below-a", [nb + 100 + i for i in range(na)], [j + 5 for j in range(nb)])]
    if na == nb:
        x = _sorted_sample(r, na, 0, 1 << 20)
        out.append(("identical", x, list(x)))
    if na <= nb:
        big = _sorted_sample(r, nb, 0, 1 << 20)
        out.append(("a-in-b", sorted(r.permutation(big)[:na].tolist()), big))
    if nb <= na:
        big = _sorted_sample(r, na, 0, 1 << 20)
        out.append(("b-in-a", big, sorted(r.permutation(big)[:nb].tolist())))
    # ids from the whole 32-bit range, 0 and 0xFFFFFFFE among them: both sets draw from one pool, so they overlap
    pool = _sorted_sample(r, na + nb + 2, 1, TOP)
    a = set(r.permutation(pool)[:max(0, na - 2)].tolist()); b = set(r.permutation(pool)[:max(0, nb - 2)].tolist())
    for s, n, first in ((a, na, 0), (b, nb, TOP)):
        for x in (first, TOP - first):
            if len(s) < n:
                s.add(x)
        for x in pool:
            if len(s) >= n:
                break
            s.add(x)
    out.append(("extreme-ids", sorted(a), sorted(b)))
    return out


def _set_problems(r, out):
    for na in SET_SIZES:
        for nb in SET_SIZES:
            if na * nb >= SET_PRODUCT_LIMIT:
                continue
            for rel, a, b in _relations(r, na, nb):
                assert len(a) == na and len(b) == nb and len(set(a)) == na and len(set(b)) == nb
                sa, sb = set(a), set(b)
                a_, b_ = np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32)
                tag = "%s na=%d nb=%d" % (rel, na, nb)
                out.append(("UNION " + tag, (api.SETS_UNION, a_, b_, 0), ("list", sorted(sa | sb))))
                out.append(("INTER " + tag, (api.SETS_INTER, a_, b_, 0), ("list", sorted(sa & sb))))
                out.append(("DIFF " + tag, (api.SETS_DIFF, a_, b_, 0), ("list", sorted(sa - sb))))
                for cap in sorted({0, 1, 2, 30, na}):
                    out.append(("INTER_COUNT cap=%d %s" % (cap, tag), (api.SETS_INTER_COUNT, a_, b_, cap), ("count", len(sa & sb), cap)))


def _sort_problems(r, out):
    for n in SORT_SIZES:
        vals = r.randint(0, 1 << 62, size=n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + r.randint(0, 2, size=n, dtype=np.int64).astype(np.uint64)  # < 2^63
        distinct = np.array(_sorted_sample(r, n, 0, 1 << 62), dtype=np.uint64)
        kinds = (("distinct", r.permutation(distinct)), ("all-equal", np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)),
                 ("bit-63", r.permutation(distinct) | np.uint64(1 << 63)), ("sorted", distinct), ("reversed", distinct[::-1].copy()))
        for kind, keys in kinds:
            pairs = sorted(zip(keys.tolist(), vals.tolist()))
            out.append(("SORT_PAIRS %s n=%d" % (kind, n), (api.SETS_SORT_PAIRS, keys, vals, 0), ("pairs", [p[0] for p in pairs], [p[1] for p in pairs])))


def _radix_problems(r, out):
    for n in RADIX_SIZES:
        for mk in RADIX_MAX_KEYS:
            keys = r.randint(0, mk + 1, size=n, dtype=np.int64)
            if n:  # the largest key decides the number of passes; a run of more than 64 equal keys spans two chunks of the stable scatter
                keys[r.randint(0, n)] = mk
            if n >= 70:
                at = r.randint(0, n - 69); keys[at:at + 70] = keys[at]
            if n >= 300:
                keys[r.permutation(n)[:100]] = mk // 2
            if n:
                keys[r.randint(0, n)] = mk
            keys = keys.astype(np.uint32)
            want = sorted(keys.tolist())
            out.append(("RADIX_U32 n=%d max_key=%d" % (n, mk), (api.SETS_RADIX_U32, keys, [], mk), ("list", want)))
            if n <= 512:  # the wide layout (second buffer in device memory) at the small sizes too: nb != 0 asks for it
                out.append(("RADIX_U32 wide n=%d max_key=%d" % (n, mk), (api.SETS_RADIX_U32, keys, [0], mk), ("list", want)))
            order = sorted(range(n), key=lambda i: keys[i])  # stable: equal keys keep their payload order
            out.append(("RADIX_PAIRS_U32 n=%d max_key=%d" % (n, mk), (api.SETS_RADIX_PAIRS_U32, keys, np.arange(n, dtype=np.uint32), mk), ("list", want + order)))


def _bm_problems(r, out):
    for U in UNIVERSES:
        uni = _sorted_sample(r, U, 0, 1 << 32)
        last = 64 * ((U - 1) // 64)
        lane0 = [i for i in range(min(64, U)) if r.randint(0, 2)] or [0]
        tail = [i for i in range(last, U) if r.randint(0, 2)] or [U - 1]
        subsets = (("empty", []), ("full", list(range(U))), ("one", [int(r.randint(0, U))]), ("lane-0-word", lane0), ("last-word", tail), ("every-7th", list(range(0, U, 7))))
        for name, idx in subsets:
            ids = [uni[i] for i in idx]
            count = len(ids)
            for q in sorted({x for x in (0, 1, count - 1, count, count + 1, 30) if x >= 0}):
                for op, opname in ((api.SETS_BM_LOWEST, "BM_LOWEST"), (api.SETS_BM8_LOWEST, "BM8_LOWEST")):
                    if op == api.SETS_BM8_LOWEST and U > 512:
                        continue
                    out.append(("%s U=%d %s q=%d" % (opname, U, name, q), (op, np.array(uni, dtype=np.uint32), np.array(ids, dtype=np.uint32), q), ("lowest", ids[:q], count)))


@functools.lru_cache(maxsize=None)
def _problems():
    r = np.random.RandomState(20250117)
    out = []
    _set_problems(r, out); _sort_problems(r, out); _radix_problems(r, out); _bm_problems(r, out)
    return out


def _check(lib, device):
    probs = _problems()
    got = api.sets_batch([p for _, p, _ in probs], lib_path=lib)
    assert len(got) == len(probs)
    bad, skipped, by_op = [], 0, {}
    for (name, (op, _, _, _), want), (words, res, st) in zip(probs, got):
        if st == api.SETS_NOT_IN_BUILD and not device and op in DEVICE_ONLY:
            skipped += 1
            continue
        by_op[op] = by_op.get(op, 0) + 1
        ok = st == api.SETS_OK
        if ok and want[0] == "list":
            ok = words == want[1] and (op not in (api.SETS_UNION, api.SETS_INTER, api.SETS_DIFF) or res == len(want[1]))
        elif ok and want[0] == "count":
            true, cap = want[1], want[2]
            ok = (res == true) if true < cap else (cap <= res <= true)
        elif ok and want[0] == "pairs":
            ok = words == (want[1], want[2])
        elif ok and want[0] == "lowest":
            ok = words == want[1] and res == want[2]
        if not ok:
            bad.append("%s: status %d result %d, %s" % (name, st, res, str(words)[:120]))
    print("%d problems in one launch, %d answered 'not in this build'; checked by operation: %s" % (len(probs), skipped, sorted(by_op.items())))
    assert not bad, "%d of %d problems differ from the reference, e.g. %s" % (len(bad), len(probs), bad[:8])
    n_device_only = sum(1 for _, p, _ in probs if p[0] in DEVICE_ONLY)
    assert skipped == (0 if device else n_device_only)  # the simulator lacks exactly the device-only operations
    assert all(by_op.get(op, 0) > 0 for op in range(9) if device or op not in DEVICE_ONLY)


def test_sim_wave_sets():
    _check(SIM_LIB, device=False)


@pytest.mark.gpu
def test_gpu_wave_sets():
    _check(None, device=True)


def test_sets_batch_refuses_what_would_write_outside_a_slice():
    """the entry checks sizes on the host: a universe above 4096 ids, ids outside the universe, more than 1664 radix keys"""
    for prob in ((api.SETS_BM_LOWEST, list(range(4097)), [1], 1), (api.SETS_BM_LOWEST, [1, 5, 9], [4], 1), (api.SETS_BM8_LOWEST, list(range(513)), [1], 1),
                 (api.SETS_RADIX_U32, list(range(1665)), [], 1 << 20), (api.SETS_SORT_PAIRS, [1, 2], [1], 0), (99, [], [], 0)):
        with pytest.raises(api.RtkError):
            api.sets_batch([prob], lib_path=SIM_LIB)
