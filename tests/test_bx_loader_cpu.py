"""The native BAM loader's linked-read rule (use_bx_tag / bxTagUpperLimit; include/quilt_amd_io.h, csrc/hostio.cpp) against two
yardsticks: hand-written expected reads for the boundary cases, and `model()` below -- the rule of the header restated in plain
Python over the list of alignments (it shares nothing with the C++: its own pile-up, its own chaining, its own resolution, its own
coverage cap).  Every generated file goes through both.  The rule is the project's own (STITCH is not in the reference tree):
these tests pin the statement in the header, not STITCH."""
import os

import numpy as np
import pytest

from tests import bamaux

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# forty sites a kilobase apart, four to a grid; reference allele A, alternate C, every other base of a read T (neither)
L = (1000 * np.arange(1, 41)).astype(np.int32)
REF, ALT = ["A"] * 40, ["C"] * 40
GRID = (np.arange(40) // 4).astype(np.int32)
REFS = [("1", 100000)]


def aln(pos, calls, name, length=20, flag=0, mapq=60, tag=None, aux=None, qual=30, tlen=0, **more):
    """An alignment pos .. pos + length - 1 (plain M) that shows `calls` {site: (allele "r" / "a", quality)}; `tag`: BX:Z"""
    seq, q = ["T"] * length, [qual] * length
    for t, (al, qq) in calls.items():
        assert pos <= L[t] < pos + length
        seq[L[t] - pos] = "C" if al == "a" else "A"
        q[L[t] - pos] = qq
    fields = list(aux or [])
    if tag is not None:
        fields.append(("BX", "Z", tag))
    return dict(ref_id=0, pos=pos, name=name, mapq=mapq, flag=flag, cigar=[(length, "M")], seq="".join(seq), qual=q, tlen=tlen,
                aux=fields, **more)


# ---------------------------------------------------------------------------------------------------------------------------
# the rule, in Python
# ---------------------------------------------------------------------------------------------------------------------------
def _stream_key(seed, i):
    M = (1 << 64) - 1
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def _pileup(a, bqFilter):
    """[(site, signed quality)] of one alignment, and its aligned span (soft clips unused)"""
    calls, q, r = [], 0, a["pos"]
    for n, op in a["cigar"]:
        if op in "M=X":
            for k in range(n):
                hit = np.flatnonzero(L == r + k)
                if len(hit):
                    t, base, bq = int(hit[0]), a["seq"][q + k], min(a["qual"][q + k], a["mapq"])
                    if bq >= bqFilter and base in (REF[t], ALT[t]):
                        calls.append((t, bq if base == ALT[t] else -bq))
            q += n
            r += n
        elif op in "IS":
            q += n
        elif op in "DN":
            r += n
    return calls, a["pos"], r - 1


def _tag(a):
    for tag, ty, val in a.get("aux", []):
        if tag == "BX":   # the first field of that name decides
            return val if ty == "Z" and val != "" else None
    return None


def model(alns, use_bx, limit, bqFilter=17, cap=0, seed=1):
    """-> (reads [(u list, bq list)] in the loader's order, the eight stats, the four BX counters)"""
    st, bx = [0] * 8, [0] * 4
    frags, by_name = [], {}
    for a in alns:
        st[0] += 1
        if a["flag"] & (0x4 | 0x100 | 0x200 | 0x400 | 0x800):
            st[4] += 1
            continue
        if a["mapq"] < bqFilter:
            st[2] += 1
            continue
        if abs(a.get("tlen", 0)) > 1000000:
            st[3] += 1
            continue
        calls, lo, hi = _pileup(a, bqFilter)
        st[1] += 1
        if not calls:
            st[7] += 1
            continue
        tag = _tag(a) if use_bx else None
        if tag is not None:
            bx[0] += 1
        if a["flag"] & 1:
            if a["name"] in by_name:
                f = frags[by_name.pop(a["name"])]
                f["alns"].append(calls)
                f["lo"], f["hi"] = min(f["lo"], lo), max(f["hi"], hi)
                st[6] += 1
                continue
            by_name[a["name"]] = len(frags)
        frags.append(dict(alns=[calls], lo=lo, hi=hi, tag=tag))
    molecules = []   # lists of fragment indices
    open_of = {}
    for i in sorted(range(len(frags)), key=lambda i: (frags[i]["lo"], i)):
        f = frags[i]
        if f["tag"] is None:
            molecules.append([i])
            continue
        m = open_of.get(f["tag"])
        if m is not None and f["lo"] - m["end"] <= limit:
            m["frags"].append(i)
            m["end"] = max(m["end"], f["hi"])
            bx[2] += 1
            continue
        if m is not None:
            bx[3] += 1
        m = dict(frags=[i], end=f["hi"])
        open_of[f["tag"]] = m
        molecules.append(m["frags"])
    slots = {}
    for m in molecules:
        bx[1] += len(m) > 1
        per_aln = [c for i in sorted(m) for c in frags[i]["alns"]]
        by_site = {}
        for calls in per_aln:
            for t, q in calls:
                by_site.setdefault(t, []).append(q)
        read = []
        for t in sorted(by_site):
            qs = by_site[t]
            if len({q < 0 for q in qs}) == 1:
                read.append((t, max(qs, key=abs)))
        if not read:
            st[7] += 1
            continue
        slots[min(m)] = read
    if cap > 0:
        depth = np.zeros(len(L), dtype=int)
        for r in slots.values():
            for t, _ in r:
                depth[t] += 1
        for t in range(len(L)):
            if depth[t] <= cap:
                continue
            for _, s in sorted((_stream_key(seed, s), s) for s, r in slots.items() if any(tt == t for tt, _ in r)):
                if depth[t] <= cap:
                    break
                for tt, _ in slots.pop(s):
                    depth[tt] -= 1
                st[5] += 1
    order = sorted(sorted(slots), key=lambda s: GRID[slots[s][(len(slots[s]) - 1) // 2][0]])   # (sorted() is stable)
    return [([t for t, _ in slots[s]], [q for _, q in slots[s]]) for s in order], st, bx


# ---------------------------------------------------------------------------------------------------------------------------
def _load(path, chr="1", sites=(L, REF, ALT, GRID), **kw):
    from quilt_amd.io import loadBamAndConvert
    s, st, bx = loadBamAndConvert(path, chr, sites[0], sites[1], sites[2], sites[3], return_stats=True, return_bx_stats=True,
                                  **{"downsampleToCov": 0, **kw})
    reads = [(s.u[a:b].tolist(), s.bq[a:b].tolist()) for a, b in zip(s.read_ptr[:-1], s.read_ptr[1:])]
    for (u, _), w in zip(reads, s.wif):   # wif: the grid of the lower-median site
        assert w == sites[3][u[(len(u) - 1) // 2]]
    return reads, list(st.values()), list(bx.values())


_N = [0]
_LAST = [None]


def written(tmp_path):
    """every BAM file the tests of this module wrote (the sanitizer test loads them all again)"""
    return sorted(str(p) for p in tmp_path.glob("case*.bam"))


def run(tmp_path, alns, limit, expect=None, sorted_header=True, **kw):
    """write, load with the tag, compare with the model (and with the hand-written reads); returns (reads, stats, bx)"""
    _N[0] += 1
    path = str(tmp_path / f"case{_N[0]:03d}.bam")
    bamaux.write_bam(path, REFS, alns, sorted_header=sorted_header)
    _LAST[0] = path
    got = _load(path, use_bx_tag=True, bxTagUpperLimit=limit, **kw)
    want = model(alns, True, limit, cap=kw.get("downsampleToCov", 0), seed=kw.get("seed", 1))
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2], (got, want)
    off = _load(path, **kw)
    want_off = model(alns, False, 0, cap=kw.get("downsampleToCov", 0), seed=kw.get("seed", 1))
    assert off[0] == want_off[0] and off[1] == want_off[1] and off[2] == [0, 0, 0, 0]
    if expect is not None:
        assert got[0] == expect, got[0]
    return got


def _same_arrays(path, chr, sites, **kw):
    from quilt_amd.io import loadBamAndConvert
    a, sa, ba = loadBamAndConvert(path, chr, *sites, return_stats=True, return_bx_stats=True, **kw)
    b, sb, bb = loadBamAndConvert(path, chr, *sites, return_stats=True, return_bx_stats=True, use_bx_tag=True, **kw)
    for name in ("read_ptr", "u", "bq", "wif"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert sa == sb and list(bb.values()) == [0, 0, 0, 0] and list(ba.values()) == [0, 0, 0, 0]
    return a, sa


def _pairs_file(path, n_pairs=300, seed=3):
    rng = np.random.default_rng(seed)
    alns = []
    for i in range(n_pairs):
        t = int(rng.integers(0, 39))
        c1 = {t: ("a" if rng.random() < 0.5 else "r", int(rng.integers(18, 40)))}
        c2 = dict(c1) if rng.random() < 0.4 else {}
        if c2 and rng.random() < 0.3:
            c2[t] = ("r" if c1[t][0] == "a" else "a", int(rng.integers(18, 40)))   # overlapping mates that disagree
        p1 = int(L[t]) - int(rng.integers(0, 20))
        if rng.random() < 0.5:
            c2[t + 1] = ("a", int(rng.integers(18, 40)))
            p2, l2 = (p1, 1100) if t in c2 else (int(L[t + 1]) - 5, 20)
        else:
            p2, l2 = (p1, 20) if c2 else (p1 + 25, 20)
        alns.append(aln(p1, c1, f"p{i}", flag=0x41, tlen=1200))
        alns.append(aln(p2, c2, f"p{i}", length=l2, flag=0x81, tlen=-1200))
    alns.sort(key=lambda a: a["pos"])
    bamaux.write_bam(path, REFS, alns)
    return alns


def test_untagged_input_changes_nothing(tmp_path):
    import json
    z = json.load(open(os.path.join(GOLD, "aligner_like.json")))
    sites = (np.array(z["sites"]["L"], dtype=np.int32), list(z["sites"]["ref"]), list(z["sites"]["alt"]), None)
    for kw in (dict(downsampleToCov=0), dict(downsampleToCov=1), dict(downsampleToCov=0, useSoftClippedBases=True)):
        s, _ = _same_arrays(os.path.join(GOLD, "aligner_like.bam"), z["chr"], sites, **kw)
    assert s.nReads > 0
    z = json.load(open(os.path.join(GOLD, "sam_spec_example.json")))
    sites = (np.array(z["sites"]["L"], dtype=np.int32), list(z["sites"]["ref"]), list(z["sites"]["alt"]), None)
    for kw in (dict(downsampleToCov=0), dict(downsampleToCov=0, useSoftClippedBases=True), dict(downsampleToCov=0, chrStart=30, chrEnd=45)):
        s, _ = _same_arrays(os.path.join(GOLD, "sam_spec_example.bam"), "ref", sites, **kw)
    b = z["expect"]["big"]
    _same_arrays(os.path.join(GOLD, "sam_spec_example.bam"), "big", (np.array(b["L"], dtype=np.int32), list(b["ref"]), list(b["alt"]), None),
                 downsampleToCov=0)
    # mate pairs (some overlapping, some disagreeing) under a coverage cap that bites
    path = str(tmp_path / "case_pairs.bam")
    alns = _pairs_file(path)
    s, st = _same_arrays(path, "1", (L, REF, ALT, GRID), downsampleToCov=5)
    assert st["removed_by_coverage_cap"] > 20 and st["mates_merged"] > 100 and st["no_site"] > 0
    want = model(alns, True, 50000, cap=5)
    got = _load(path, use_bx_tag=True, downsampleToCov=5)
    assert got[0] == want[0] and got[1] == want[1]


def test_limit_boundary(tmp_path):
    a = aln(990, {0: ("a", 30)}, "a", tag="X")      # 990 .. 1009
    b = aln(1990, {1: ("r", 31)}, "b", tag="X")     # gap 1990 - 1009 = 981
    _, _, bx = run(tmp_path, [a, b], 981, expect=[([0, 1], [30, -31])])
    assert bx == [2, 1, 1, 0]
    _, _, bx = run(tmp_path, [a, b], 980, expect=[([0], [30]), ([1], [-31])])
    assert bx == [2, 0, 0, 1]
    # the same tag meets again after a split: [A] [B, C]
    b = aln(2990, {2: ("r", 31)}, "b", tag="X")     # gap 1981
    c = aln(3990, {3: ("a", 32)}, "c", tag="X")     # gap 3990 - 3009 = 981
    _, _, bx = run(tmp_path, [a, b, c], 1000, expect=[([0], [30]), ([2, 3], [-31, 32])])
    assert bx == [3, 1, 1, 1]
    run(tmp_path, [a, b, c], 0, expect=[([0], [30]), ([2], [-31]), ([3], [32])])
    run(tmp_path, [a, b, c], 50000, expect=[([0, 2, 3], [30, -31, 32])])


def test_chaining_runs_from_the_largest_end(tmp_path):
    long = aln(990, {0: ("a", 30)}, "long", length=3000, tag="X")   # 990 .. 3989
    short = aln(1990, {1: ("a", 31)}, "short", tag="X")             # inside it, ends at 2009
    third = aln(4990, {4: ("r", 32)}, "third", tag="X")             # 1001 past the long one's end, 2981 past the short one's
    run(tmp_path, [long, short, third], 1001, expect=[([0, 1, 4], [30, 31, -32])])
    run(tmp_path, [long, short, third], 1000, expect=[([0, 1], [30, 31]), ([4], [-32])])


def test_interleaved_tags(tmp_path):
    alns = [aln(990, {0: ("a", 30)}, "x1", tag="X"), aln(1990, {1: ("r", 31)}, "y1", tag="Y"),
            aln(2990, {2: ("r", 32)}, "x2", tag="X"), aln(3990, {3: ("a", 33)}, "y2", tag="Y")]
    _, _, bx = run(tmp_path, alns, 5000, expect=[([0, 2], [30, -32]), ([1, 3], [-31, 33])])
    assert bx == [4, 2, 2, 0]
    # haplotagging's "00 segment = invalid barcode" convention is NOT applied: such a value is a barcode like any other
    alns = [aln(990, {0: ("a", 30)}, "x1", tag="A00C00B00D00"), aln(1990, {1: ("r", 31)}, "x2", tag="A00C00B00D00")]
    run(tmp_path, alns, 5000, expect=[([0, 1], [30, -31])])


def test_resolution_at_a_shared_site(tmp_path):
    def trio(c1, c2, c3, more=True):
        extra = {1: ("r", 22)} if more else {}
        return [aln(985, {0: c1}, "p", flag=0x41, tag="X", tlen=30), aln(990, {0: c2}, "p", flag=0x81, tag="X", tlen=-30),
                aln(995, {0: c3, **extra}, "s", length=1100 if more else 20, tag="X")]
    # all agree: the highest quality
    _, st, bx = run(tmp_path, trio(("a", 20), ("a", 35), ("a", 25)), 100, expect=[([0, 1], [35, -22])])
    assert st[6] == 1 and bx == [3, 1, 1, 0]
    # two agree, one disagrees (whichever it is): the site is dropped
    run(tmp_path, trio(("a", 30), ("a", 35), ("r", 20)), 100, expect=[([1], [-22])])
    run(tmp_path, trio(("a", 30), ("r", 30), ("a", 20)), 100, expect=[([1], [-22])])   # (mate by mate, then the third, would keep it)
    # a tie: one call of that quality
    run(tmp_path, trio(("r", 30), ("r", 30), ("r", 28)), 100, expect=[([0, 1], [-30, -22])])
    # the only site dropped: not a read
    _, st, _ = run(tmp_path, trio(("a", 30), ("a", 35), ("r", 20), more=False), 100, expect=[])
    assert st[7] == 1


def test_untagged_stays_untagged(tmp_path):
    pair = [aln(990, {0: ("a", 30)}, "p", flag=0x41, tlen=1100), aln(1990, {1: ("r", 25)}, "p", flag=0x81, tlen=-1100)]
    single = [aln(995, {0: ("r", 33)}, "s1"), aln(1995, {1: ("a", 34)}, "s2")]
    empty = [aln(2990, {2: ("a", 30)}, "e1", tag=""), aln(2995, {2: ("a", 31)}, "e2", tag="")]
    other = [aln(3990, {3: ("a", 30)}, "i1", aux=[("BX", "i", 7)]), aln(3995, {3: ("a", 31)}, "i2", aux=[("BX", "i", 7)])]
    alns = sorted(pair + single + empty + other, key=lambda a: a["pos"])
    _, st, bx = run(tmp_path, alns, 50000, expect=[([0, 1], [30, -25]), ([0], [-33]), ([1], [34]), ([2], [30]), ([2], [31]), ([3], [30]),
                                                   ([3], [31])])
    assert bx == [0, 0, 0, 0] and st[6] == 1


def test_filters_come_first(tmp_path):
    a = aln(990, {0: ("a", 30)}, "a", tag="X")
    c = aln(2990, {2: ("a", 32)}, "c", tag="X")      # 1981 past a: joins a only through something in between
    for bridge in (aln(1990, {1: ("a", 31)}, "b", tag="X", flag=0x400),          # duplicate
                   aln(1990, {1: ("a", 31)}, "b", tag="X", mapq=10),             # mapping quality below bqFilter
                   aln(1990, {1: ("a", 10)}, "b", tag="X"),                      # its only base is below bqFilter: no site
                   aln(1500, {}, "b", tag="X")):                                 # between the sites: no site
        _, _, bx = run(tmp_path, [a, bridge, c], 1000, expect=[([0], [30]), ([2], [32])])
        assert bx == [2, 0, 0, 1]
    run(tmp_path, [a, aln(1990, {1: ("a", 31)}, "b", tag="X"), c], 1000, expect=[([0, 1, 2], [30, 31, 32])])


def test_unsorted_file_equals_its_sorted_twin(tmp_path):
    rng = np.random.default_rng(8)
    alns = []
    for i in range(60):
        t = int(rng.integers(0, 40))
        alns.append(aln(int(L[t]) - int(rng.integers(0, 15)), {t: ("a" if rng.random() < 0.5 else "r", int(rng.integers(18, 40)))}, f"r{i}",
                        tag=[None, "X", "Y", "Z"][int(rng.integers(0, 4))]))
    twin = sorted(alns, key=lambda a: a["pos"])
    shuffled = [alns[i] for i in rng.permutation(len(alns))]
    a, _, bxa = run(tmp_path, twin, 3000)
    b, _, bxb = run(tmp_path, shuffled, 3000, sorted_header=False)
    # (the order of reads inside one grid is the file's order, with or without the tag: the molecules are compared as a set)
    assert sorted(a) == sorted(b) and bxa == bxb and bxa[1] > 3 and bxa[3] > 0


EVERY_TYPE = [("XA", "A", "q"), ("Xc", "c", -3), ("XC", "C", 200), ("Xs", "s", -300), ("XS", "S", 60000), ("Xi", "i", -70000),
              ("XI", "I", 4000000000), ("Xf", "f", 1.5), ("XZ", "Z", "text"), ("XH", "H", "1AE301"), ("Bc", "B", ("c", [-1, 2, 3])),
              ("BC", "B", ("C", [1, 2, 250])), ("Bs", "B", ("s", [-1000, 7])), ("BS", "B", ("S", [65535])), ("Bi", "B", ("i", [-5, 6])),
              ("BI", "B", ("I", [4000000000, 1])), ("Bf", "B", ("f", [0.25, 2.0, -1.0])), ("B0", "B", ("C", []))]


def test_auxiliary_walk(tmp_path):
    one = [([0, 1], [30, -31])]
    # BX behind one field of every type (and behind all of them at once)
    for fields in [[f] for f in EVERY_TYPE] + [EVERY_TYPE]:
        alns = [aln(990, {0: ("a", 30)}, "a", aux=fields, tag="X"), aln(1990, {1: ("r", 31)}, "b", aux=fields, tag="X")]
        run(tmp_path, alns, 5000, expect=one)
    # the long-CIGAR form (CG:B,I behind the <l_seq>S<ref_len>N placeholder) with a BX tag, in either order: both are honoured
    for bx_first in (False, True):
        a = aln(990, {0: ("a", 30)}, "a", tag="X", placeholder=True)   # (bamaux puts CG in front of the other fields)
        if bx_first:
            a = aln(990, {0: ("a", 30)}, "a", aux=[("BX", "Z", "X"), ("CG", "B", ("I", [(20 << 4) | 0]))])
            a["cigar"] = [(20, "S"), (20, "N")]
        b = aln(1990, {1: ("r", 31)}, "b", tag="X")
        path = str(tmp_path / f"case_cg{int(bx_first)}.bam")
        bamaux.write_bam(path, REFS, [a, b])
        reads, st, bx = _load(path, use_bx_tag=True, bxTagUpperLimit=5000)
        assert reads == one and bx == [2, 1, 1, 0]
        assert _load(path)[0] == [([0], [30]), ([1], [-31])]
    # a record cut inside its auxiliary data: no fault, and the alignment is untagged unless its BX field is whole
    alns = [aln(990, {0: ("a", 30)}, "a", tag="X"), aln(1990, {1: ("r", 31)}, "b", aux=[("Xi", "i", 5), ("Bs", "B", ("s", [1, 2]))], tag="X")]
    full = len(bamaux.aux_bytes(alns[1]["aux"]))
    for cut in range(full + 1):
        path = str(tmp_path / f"case_cut{cut:02d}.bam")
        bamaux.write_bam(path, REFS, alns, cut_last_aux=cut)
        reads, _, bx = _load(path, use_bx_tag=True, bxTagUpperLimit=5000)
        assert reads == (one if cut == full else [([0], [30]), ([1], [-31])]), cut
        assert bx[0] == (2 if cut == full else 1)
        assert _load(path)[0] == [([0], [30]), ([1], [-31])]


def test_cap_and_order(tmp_path):
    """A cap of 2 at a site three reads cover, one of them a molecule: the molecule counts once, and the reads outside it are kept
    or removed exactly as without the tag (their slots, hence their stream keys, do not move)."""
    alns = [aln(990, {0: ("a", 30)}, "m1", tag="X"), aln(992, {0: ("r", 31)}, "s1"), aln(994, {0: ("a", 32)}, "s2"),
            aln(1990, {1: ("r", 33)}, "m2", tag="X"), aln(4990, {4: ("a", 34)}, "far")]
    outcomes = set()
    for seed in range(1, 9):
        on, st, _ = run(tmp_path, alns, 5000, downsampleToCov=2, seed=seed)
        off, st_off, _ = _load(_LAST[0], downsampleToCov=2, seed=seed)
        assert st[5] == st_off[5] == 1
        molecule_kept = ([0, 1], [30, -33]) in on
        outcomes.add(molecule_kept)
        assert molecule_kept == (([0], [30]) in off)           # the molecule lives in its first fragment's slot
        singles = lambda reads: [r for r in reads if r in (([0], [-31]), ([0], [32]), ([4], [34]))]
        assert singles(on) == singles(off)
        assert len(on) == 3 and (molecule_kept or ([1], [-33]) not in on)   # (removed, the molecule goes whole)
    assert outcomes == {True, False}


def test_bad_limit(tmp_path):
    from quilt_amd.io import loadBamAndConvert
    from quilt_amd.native import QuiltAmdError
    for path in (str(tmp_path / "does_not_exist.bam"), os.path.join(GOLD, "aligner_like.bam")):   # (refused before the file is opened)
        for use in (False, True):
            with pytest.raises(QuiltAmdError) as ei:
                loadBamAndConvert(path, "1", L, REF, ALT, GRID, use_bx_tag=use, bxTagUpperLimit=-1)
            assert "status -2" in str(ei.value)


# ---------------------------------------------------------------------------------------------------------------------------
# the auxiliary walk under AddressSanitizer + UBSan, as a stand-alone program (tests/c/bx_loader_san.cpp)
# ---------------------------------------------------------------------------------------------------------------------------
def _sanitizer_works(tmp_path):
    import subprocess
    src = tmp_path / "probe.cpp"
    src.write_text("int main(){ return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")], capture_output=True)
    return r.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True,
                                                 env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0")).returncode == 0


def test_loader_is_clean_under_the_sanitizers(tmp_path):
    """csrc/hostio.cpp alone (no device runtime) behind tests/c/bx_loader_san.cpp, built with g++ -fsanitize=address,undefined:
    every file the tests above write, and a copy of each cut at every byte of its last record's auxiliary data, loaded with the tag
    off and on.  A clean exit, no report."""
    import shutil
    import subprocess
    if shutil.which("g++") is None or not _sanitizer_works(tmp_path):
        pytest.skip("no working g++ -fsanitize=address,undefined here")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "bx_loader_san"
    build = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g1", "-O0",
                            "-std=c++17", os.path.join(root, "quilt_amd", "csrc", "hostio.cpp"), os.path.join(root, "tests", "c", "bx_loader_san.cpp"),
                            os.path.join(root, "tests", "c", "bx_loader_stubs.cpp"), "-lz", "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    files = tmp_path / "files"
    files.mkdir()
    for test in (test_limit_boundary, test_chaining_runs_from_the_largest_end, test_interleaved_tags, test_resolution_at_a_shared_site,
                 test_untagged_stays_untagged, test_filters_come_first, test_unsorted_file_equals_its_sorted_twin, test_auxiliary_walk,
                 test_cap_and_order):
        test(files)
    _pairs_file(str(files / "case_pairs.bam"), n_pairs=40)
    paths = written(files)
    assert len(paths) > 60
    cuts = []
    for p in paths:
        cuts += bamaux.cut_copies(p, p[:-4])
    assert len(cuts) > 500
    with open(tmp_path / "sites.bin", "wb") as f:
        f.write(np.int32(len(L)).tobytes() + L.tobytes() + "".join(REF).encode() + "".join(ALT).encode() + GRID.tobytes())
    with open(tmp_path / "list.txt", "w") as f:
        f.write("\n".join(paths + cuts) + "\n")
    run_ = subprocess.run([str(exe), str(tmp_path / "sites.bin"), str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1"))
    for mark in ("AddressSanitizer", "runtime error:"):
        assert mark not in run_.stderr, run_.stderr[-6000:]
    assert run_.returncode == 0, (run_.returncode, run_.stderr[-3000:])
    assert f"bx loader: ok, {len(paths) + len(cuts)} files" in run_.stdout
