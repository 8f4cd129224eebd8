"""What `rtk_build_index --cover-edges-from` costs and what it changes (profiles/index_cover_edges.txt; DESIGN.md section 4 [A16]). The 60 Mb set of
profiles/index_graph_reuse.txt (rtk_simulate --seed 2 --ref-len 60000000 --het 0.001, short reads sampled at 30x), k = 31 with --subsample-colours, the k1 graph
taken from the k2 unitig file of --graph-only, which is also the cover file -- the command line `correct -s ... --k1-from-k2 --cover-edges` gives its k1 index step.
  python profiles/scripts/index_cover_edges.py --work DIR [--runs 5] [--parent-tool PATH/bin/rtk_build_index] [--host fast|plain] [--effect] >> profiles/index_cover_edges.txt
--host fast|plain: the lap of that host route only (no GPU needed); default: the --gpu laps and walls, alternating with the parent's tool when given.
--effect: the one-command run with and without --cover-edges, reads whose output differs, identity of both outputs to the simulated truth (needs the GPU)."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "ratatosk_amd", "bin")
LAP = re.compile(r"rtk_build_index: \[ *([0-9.]+) s\] (.*)")
COUNTS = re.compile(r"cover: edges_recorded=(\d+) edges_covered=(\d+) ids_added=(\d+)")
STAGE = re.compile(r"rtk_index_cover: .*")
ENV = dict(os.environ, RTK_INDEX_TRACE="1", RTK_INDEX_THREADS="16")


def build(tool, args, timeout):
    t0 = time.time()
    r = subprocess.run([tool] + args, capture_output=True, text=True, env=ENV, timeout=timeout)
    wall = time.time() - t0
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    laps, prev = {}, 0.0
    for m in LAP.finditer(r.stderr):
        laps[m.group(2)] = float(m.group(1)) - prev
        prev = float(m.group(1))
    return dict(wall=wall, laps=laps, err=r.stderr)


def med(v):
    return "median %.2f (%s) spread %.2f" % (statistics.median(v), " ".join("%.2f" % x for x in v), max(v) - min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True); ap.add_argument("--parent-tool"); ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host", choices=["fast", "plain"]); ap.add_argument("--effect", action="store_true"); ap.add_argument("--lr-n", type=int, default=2000)
    ap.add_argument("--ref-len", type=int, default=60000000)
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    tool, pre = os.path.join(BIN, "rtk_build_index"), os.path.join(a.work, "c2")
    if not os.path.exists(pre + ".ref.fa"):
        subprocess.check_call([os.path.join(BIN, "rtk_simulate"), "--prefix", pre, "--seed", "2", "--ref-len", str(a.ref_len), "--het", "0.001", "--sr-cov", "0",
                               "--lr-n", str(a.lr_n), "--lr-len", "8000", "--lr-profile", "ont", "--lr-err", "0.07", "--lr-truth"], stderr=subprocess.DEVNULL, timeout=600)
    sr = "sample:%s.ref.fa?cov=30&len=150&insert=500&err=0.005&seed=2" % pre
    g = os.path.join(a.work, "g")
    graph = g + ".index.k63.fasta.gz"
    route = {"fast": ["--fast"], "plain": [], None: ["--gpu"]}[a.host]
    if not os.path.exists(graph):
        build(tool, ["--graph-only", "-k", "63", "-s", sr, "-o", g] + (route if a.host != "plain" else ["--fast"]), 1500)
    common = ["--graph-from", graph, "-k", "31", "-s", sr, "--snps", "--subsample-colours"]
    out = os.path.join(a.work, "o")
    if a.host:
        print("== host route %s, %d hardware threads, no GPU: rtk_build_index %s --graph-from G -k 31 -s SR --snps --subsample-colours --cover-edges-from G" % (a.host if a.host == "plain" else "--fast", os.cpu_count() or 0, " ".join(route)))
        rs = []
        for _ in range(a.runs):
            rs.append(build(tool, common + route + ["--cover-edges-from", graph, "-o", out + "_h" + a.host], 3000))
            print("  run %d: lap 'low-coverage edges covered' %.2f s, wall %.1f s" % (len(rs), rs[-1]["laps"].get("low-coverage edges covered", 0.0), rs[-1]["wall"])); sys.stdout.flush()
        print("  lap 'low-coverage edges covered': " + med([r["laps"].get("low-coverage edges covered", 0.0) for r in rs]))
        print("  counts: edges recorded %s, edges covered %s, ids added %s" % COUNTS.search(rs[-1]["err"]).groups())
        return
    if not a.effect:
        print("== --gpu, one MI355X, 16 host threads: rtk_build_index --gpu --graph-from G -k 31 -s SR --snps --subsample-colours [--cover-edges-from G]; %d runs each, alternating" % a.runs)
        rows = {"parent, without the option": [], "without the option": [], "--cover-edges-from": []}
        for _ in range(a.runs):
            if a.parent_tool:
                rows["parent, without the option"].append(build(a.parent_tool, common + ["--gpu", "-o", out + "_p"], 600))
            rows["without the option"].append(build(tool, common + ["--gpu", "-o", out + "_n"], 600))
            rows["--cover-edges-from"].append(build(tool, common + ["--gpu", "--cover-edges-from", graph, "-o", out + "_c"], 600))
        for name, rs in rows.items():
            if rs:
                print("  %-28s wall s: %s" % (name, med([r["wall"] for r in rs])))
        cs = rows["--cover-edges-from"]
        print("  lap 'low-coverage edges covered': " + med([r["laps"].get("low-coverage edges covered", 0.0) for r in cs]))
        print("  counts: edges recorded %s, edges covered %s, ids added %s" % COUNTS.search(cs[-1]["err"]).groups())
        print("  | " + STAGE.search(cs[-1]["err"]).group(0))
        same = lambda x, y: all(open(out + x + e, "rb").read() == open(out + y + e, "rb").read() for e in (".index.k31.fasta.gz", ".index.k31.rtsk"))
        if a.parent_tool:
            print("  files without the option against the parent's: %s" % ("the same bytes" if same("_p", "_n") else "DIFFERENT"))
        for h in ("fast", "plain"):
            if os.path.exists(out + "_h" + h + ".index.k31.rtsk"):
                print("  files of --gpu against the %s route's: %s" % (h, "the same bytes" if same("_c", "_h" + h) else "DIFFERENT"))
        return
    # the effect, once: the one-command run without and with the flag
    from ratatosk_amd import api
    from oracle import oracle_py as op
    exe, lr = os.path.join(BIN, "Ratatosk"), pre + ".lr.fq"
    rcs = lambda x: x[::-1].translate(str.maketrans("ACGT", "TGCA"))
    ref = [l for l in open(pre + ".ref.fa").read().split("\n") if l and l[0] != ">"]
    truth = []
    for l in open(pre + ".lr.truth.tsv").read().splitlines():
        _, hap, start, ln, strand = l.split("\t")
        s = ref[int(hap)][int(start):int(start) + int(ln)]
        truth.append(rcs(s) if strand.strip() == "-" else s)
    tot = sum(len(t) for t in truth)
    got = {}
    print("== the effect, once: Ratatosk correct -c 16 --gpus 1 -s SR -l LR -o OUT --subsample-colours --k1-from-k2 [--cover-edges]; %d long reads of 8 kb" % len(truth))
    for name, extra in (("without --cover-edges", []), ("with --cover-edges", ["--cover-edges"])):
        o = os.path.join(a.work, "e%d" % len(extra))
        t0 = time.time()
        r = subprocess.run([exe, "correct", "-c", "16", "--gpus", "1", "-s", sr, "-l", lr, "-o", o, "--subsample-colours", "--k1-from-k2"] + extra, capture_output=True, text=True, env=ENV, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stderr)
        m = COUNTS.search(r.stderr)
        got[name] = [x[1] for x in op.read_fastq(o + ".fastq")]
        d = sum(x[0] for x in api.myers_batch(got[name], truth, [-1] * len(truth), [0] * len(truth)))
        print("  %-22s wall %.1f s; mean identity to the truth %.6f%s" % (name, time.time() - t0, 1.0 - d / tot, "; k1 index step: edges recorded %s, covered %s, ids added %s" % m.groups() if m else ""))
    a_, b_ = got["without --cover-edges"], got["with --cover-edges"]
    print("  reads whose output differs: %d of %d" % (sum(x != y for x, y in zip(a_, b_)), len(a_)))


if __name__ == "__main__":
    main()
