"""trim-paf inputs the oracle accepts, and the ways the tests print trim-paf's results.

random_trim_paf builds a PAF file one query group at a time and keeps a group only if the oracle CLI exits 0 on that group alone under
every configuration asked for: trim-paf's query groups are independent, and a file of random irregular records as a whole almost always
holds one the reference panics on.  The groups are built to reach what the composition of trim-paf's device steps gets wrong most easily:
deep groups (many deferred passes), irregular CIGARs (the serial pair kernel, clips copied behind the ops), contained and identical spans,
touching spans, equal overlaps (tie order), q_st = 0 with a leading op that consumes no query, and names whose byte order is not their
numeric order."""
import functools

import numpy as np

from rbtest_util import OPCH, QRY, random_cigar, sums, unpack

# one trim-paf configuration: the oracle's arguments, rb's (short options), and what the Python drivers take
CONFIGS = {
    "default": dict(pre=[], opts=[], rb_opts=[], scores=(1, 1, 1), policy=0, remove=False),
    "legacy": dict(pre=["--bsearch", "legacy"], opts=[], rb_opts=[], scores=(1, 1, 1), policy=1, remove=False),
    "scores": dict(pre=[], opts=["--match-score", "2", "--diff-score", "3", "--indel-score", "5"], rb_opts=["-m", "2", "-d", "3", "-i", "5"],
                   scores=(2, 3, 5), policy=0, remove=False),
    "remove": dict(pre=[], opts=["-r"], rb_opts=["-r"], scores=(1, 1, 1), policy=0, remove=True),
}

MODES = ("regular", "indel_ends", "spliced", "wild")


def oracle_args(cfg, path="-"):
    c = CONFIGS[cfg]
    return [*c["pre"], "trim-paf", *c["opts"], path]


def rb_args(cfg, path="-"):
    c = CONFIGS[cfg]
    return [*c["pre"], "trim-paf", *c["rb_opts"], path]


def _cg(ops):
    return "".join(f"{int(v) >> 4}{OPCH[int(v) & 15]}" for v in ops)


def _names(rng, n):
    """n distinct query names: numbers whose byte order differs from their numeric order (q9 > q10), names that are prefixes of others
    (q1, q10, q100, q1_alt), mixed case (Q1 < q1).  Most share the prefix 'q', so a cut of the sorted names falls between two of them."""
    out, seen = [], set()
    pool = [1, 2, 9, 10, 11, 19, 99, 100, 101, 1000]
    while len(out) < n:
        r = rng.random()
        if r < .7:
            nm = f"q{int(rng.choice(pool)) if rng.random() < .5 else int(rng.integers(0, 400))}"
        elif r < .8:
            nm = f"Q{int(rng.choice(pool))}"
        elif r < .9:
            nm = f"q{int(rng.choice(pool))}_alt"
        else:
            nm = f"q{int(rng.choice(pool))}.{int(rng.integers(1, 3))}"
        if nm not in seen:
            seen.add(nm)
            out.append(nm)
    return out


def _record(rng, recs, tie_ov, p_mode):
    """(q_st, cigar) of one more record of a group whose records so far are `recs`"""
    mode = str(rng.choice(MODES, p=p_mode))
    c = random_cigar(rng, int(rng.integers(3, 50)), mode)
    if mode == "wild" and rng.random() < .5 and (int(c[0]) & 15) in QRY:   # a leading op that consumes no query (the replay corner)
        c = np.r_[np.uint32((int(rng.integers(1, 4)) << 4) | int(rng.choice([2, 3, 5, 6]))), c]
    if sums(c)[1] < 2:
        c = np.r_[c, np.uint32((20 << 4) | 7)]
    q = sums(c)[1]
    if not recs:
        return (0 if rng.random() < .35 else int(rng.integers(0, 300))), c
    p_st, p_c = recs[int(rng.integers(0, len(recs)))]
    p_q = sums(p_c)[1]
    p_en = p_st + p_q
    rel = rng.random()
    if rel < .08:                                   # identical span (same cigar, same start)
        return p_st, p_c.copy()
    if rel < .16 and q < p_q:                       # contained
        return p_st + int(rng.integers(0, p_q - q + 1)), c
    if rel < .24:                                   # touching: zero overlap
        return p_en, c
    if rel < .5 and tie_ov < min(p_q, q):           # the group's common overlap: ties
        return p_en - tie_ov, c
    if rel < .56:                                   # the same start as another record (q_st = 0 again, often)
        return p_st, c
    return max(0, p_en - int(rng.integers(1, max(2, min(p_q, q))))), c


def _lines(name, recs, q_len):
    lines = []
    for qs, c, ts, strand, t, nm, mq in recs:
        R, Q = sums(c)
        lines.append(f"{name}\t{q_len}\t{qs}\t{qs + Q}\t{strand}\t{t}\t200000\t{ts}\t{ts + R}\t{nm}\t{max(R, Q)}\t{mq}\tcg:Z:{_cg(c)}\n")
    return lines


def _group(rng, name, size, accepted, tries=30):
    """the lines of one query group of `size` records, built one record at a time: a record is kept if `accepted` (the oracle on the group
    so far) says yes, so that deep groups, whose records all take part in pairs, are reachable at all"""
    wild_p = .25 if size <= 12 else .12
    p_mode = np.array([.4, .2, .15, wild_p])
    p_mode /= p_mode.sum()
    tie_ov = int(rng.integers(1, 12))
    q_len = 0
    recs = []
    for _ in range(size):
        for _ in range(tries):
            qs, c = _record(rng, [(r[0], r[1]) for r in recs], tie_ov, p_mode)
            R = sums(c)[0]
            rec = (qs, c, 0 if rng.random() < .3 else int(rng.integers(0, 100_000)), "+" if rng.random() < .5 else "-",
                   f"t{int(rng.integers(1, 4))}", int(rng.integers(0, R + 1)), int(rng.integers(0, 61)))
            ql = max(q_len, qs + sums(c)[1] + int(rng.integers(0, 50)))
            lines = _lines(name, recs + [rec], ql)
            if accepted("".join(lines).encode()):
                recs.append(rec)
                q_len = ql
                break
        else:
            return None
    return _lines(name, recs, q_len)


def group_sizes(rng, n_groups):
    """one of 40 or more (first: it sets how many passes the file takes), three of 12, 1, 2, 3, the rest small"""
    fixed = [int(rng.integers(40, 56)), 12, 12, 12, 1, 2, 3]
    rest = [int(x) for x in rng.choice([1, 2, 2, 3, 3, 4, 5, 6, 8], max(0, n_groups - len(fixed)))]
    return fixed + rest


@functools.lru_cache(maxsize=None)
def trim_file(seed, n_groups=150):
    """random_trim_paf under every configuration, once per process"""
    return random_trim_paf(seed, n_groups)


def random_trim_paf(seed, n_groups, configs=tuple(CONFIGS), oracle=None, tries=8):
    """PAF text (bytes) of n_groups query groups, each of which the oracle CLI runs to exit 0 on its own under every configuration in
    `configs` (names of CONFIGS).  The lines of different groups are interleaved in the file (the reference sorts them stably by name)."""
    if oracle is None:
        from oracle import pyoracle as oracle
    rng = np.random.default_rng(seed)
    names = _names(rng, n_groups)
    ok = lambda text: all(oracle.cli(*oracle_args(c), stdin=text)[0] == 0 for c in configs)  # noqa: E731

    def group(name, size):
        for _ in range(tries):
            lines = _group(rng, name, size, ok)
            if lines is not None:
                return lines
        raise RuntimeError(f"seed {seed}: no group of {size} records for {name} that the oracle accepts")

    sizes = group_sizes(rng, n_groups)
    groups = [group(name, size) for name, size in zip(names, sizes)]
    # the groups are independent but for one thing: every pass strips the trailing indels of EVERY record (paf.rs:218-220), so a deeper
    # group elsewhere can give a group's clips one more strip than it had alone.  The first group after which a prefix of the file panics
    # is made again (rarely needed)
    text = lambda gs: "".join("".join(g) for g in gs).encode()  # noqa: E731
    for _ in range(20):
        if ok(text(groups)):
            break
        lo, hi = 0, len(groups)  # prefix lo passes, prefix hi does not
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if ok(text(groups[:mid])) else (lo, mid)
        groups[hi - 1] = group(names[hi - 1], sizes[hi - 1])
    else:
        raise RuntimeError(f"seed {seed}: the oracle keeps panicking on the whole file")
    # interleave: the groups' lines in a random order that keeps each group's own order
    slots = np.repeat(np.arange(len(groups)), [len(g) for g in groups])
    rng.shuffle(slots)
    pos = [0] * len(groups)
    out = []
    for g in slots:
        out.append(groups[g][pos[g]])
        pos[g] += 1
    out = "".join(out).encode()
    assert ok(out)
    return out


@functools.lru_cache(maxsize=None)
def pipeline_file(seed, n_groups=150, max_size=100):
    """the groups of trim_file(seed) on which the oracle's `trim-paf | break-paf --max-size 100 -` (the README pipeline) exits 0: break-paf
    panics on records trim-paf passes through (a file of irregular records as a whole almost always holds one)"""
    from oracle import pyoracle as oracle
    text = trim_file(seed, n_groups)
    groups = {}
    for ln in text.splitlines(keepends=True):
        groups.setdefault(ln.split(b"\t")[0], []).append(ln)

    def ok(t):
        rc, trimmed = oracle.cli("trim-paf", "-", stdin=t)
        return rc == 0 and oracle.cli("break-paf", "--max-size", str(max_size), "-", stdin=trimmed)[0] == 0

    keep = {q for q, g in groups.items() if ok(b"".join(g))}
    out = b"".join(ln for ln in text.splitlines(keepends=True) if ln.split(b"\t")[0] in keep)
    assert ok(out)
    return out


def panic_group():
    """one group the oracle panics on under every configuration, in the pair step (both records pass remove_trailing_indels): q_st = 0 on
    '+' behind a leading op that consumes no query, and the cut finds no base (status 16)"""
    return (b"p1\t123\t0\t62\t+\tt1\t200000\t0\t64\t26\t64\t55\tcg:Z:3N3M7=40=7=1I2=2=\n"
            b"p1\t123\t51\t80\t-\tt3\t200000\t81889\t82064\t36\t175\t15\tcg:Z:1=3I1=3X2=1X1I1=3X9=150D3X1=\n")


def parse(text):
    """PAF text -> list of record dicts (the host driver's input form); the columns a route must print come along"""
    from rbtest_util import pack
    out = []
    for ln in text.decode().splitlines():
        t = ln.split("\t")
        cg = [x for x in t[12:] if x.startswith("cg:Z:")]
        out.append(dict(q_name=t[0], q_len=int(t[1]), q_st=int(t[2]), q_en=int(t[3]), strand=ord(t[4]), t_name=t[5], t_len=int(t[6]),
                        t_st=int(t[7]), t_en=int(t[8]), mapq=int(t[11]), cigar=pack(cg[0][5:]) if cg else np.zeros(0, np.uint32), id=""))
    return out


def paf_line(q_name, q_len, q_st, q_en, strand, t_name, t_len, t_st, t_en, nmatch, aln_len, mapq, rid, cigar):
    """one line as trim-paf prints it (the fixture's tags are dropped: id:Z: and cg:Z: only)"""
    return "\t".join(map(str, [q_name, q_len, q_st, q_en, chr(strand), t_name, t_len, t_st, t_en, nmatch, aln_len, mapq,
                               "id:Z:" + rid, "cg:Z:" + unpack(cigar)])) + "\n"


def format_recs(recs):
    """trim_driver.overlapping_paf_recs's records as trim-paf prints them"""
    return "".join(paf_line(x["q_name"], x["q_len"], x["q_st"], x["q_en"], x["strand"], x["t_name"], x["t_len"], x["t_st"], x["t_en"],
                            x["nmatch"], x["aln_len"], x["mapq"], x["id"], x["cigar"]) for x in recs)


def format_resident(r, norm0, norm, ops, new_off, order, keep=None):
    """a trim_driver.ResidentTrim's batch as trim-paf prints it: r = the input (rbtest_util.Recs), norm0 = the norm rows before the passes
    (the _TO. tag of what remove_trailing_indels stripped), norm / ops / new_off = T.gather()'s dense batch, order = T.order, keep = which
    records are printed (-r: ~T.contained)"""
    lines = []
    for i in order:
        if keep is not None and not keep[i]:
            continue
        rid = ""
        if norm0[i]["lead_ops"] or norm0[i]["trail_ops"]:
            c = r.cigars[i]
            lead, trail = c[:norm0[i]["lead_ops"]], c[len(c) - norm0[i]["trail_ops"]:][::-1]
            rid = f"_TO.{unpack(lead)}.{unpack(trail)}"
        lines.append(paf_line(r.q_name[i], r.q_len[i], int(norm[i]["q_st"]), int(norm[i]["q_en"]), r.strand[i], r.t_name[i], r.t_len[i],
                              int(norm[i]["t_st"]), int(norm[i]["t_en"]), int(norm[i]["nmatch"]), int(norm[i]["aln_len"]), r.mapq[i], rid,
                              ops[int(new_off[i]):int(new_off[i + 1])]))
    return "".join(lines)


class OracleEngine:
    """The two engine calls trim_driver.overlapping_paf_recs makes, served by the oracle's library: runs the host driver's bookkeeping on
    the CPU (tests of the driver itself and of the formatting, not of any kernel)."""

    def __init__(self, oracle):
        self.o = oracle

    def scan_records(self, ops, op_off, t_st, t_en, q_st, q_en, strand):
        b = self.o.Batch(ops, op_off, t_st, t_en, q_st, q_en, strand)
        return self.o.reduce(b), self.o.normalize(b)

    def overlap_split(self, ops, op_off, t_st, t_en, q_st, q_en, strand, left, right, scores=(1, 1, 1), policy=0):
        return self.o.overlap_split(self.o.Batch(ops, op_off, t_st, t_en, q_st, q_en, strand), left, right, scores, policy)


def is_regular(ops):
    """RB_F_REGULAR (include/rustybam_amd.h): only M I D N = X, every length >= 1, no two adjacent ops of one type, M / = / X at both
    ends -- what the pair kernels other than the serial one take"""
    c, ln = [int(v) & 15 for v in ops], [int(v) >> 4 for v in ops]
    return bool(c) and all(x in (0, 1, 2, 3, 7, 8) for x in c) and min(ln) >= 1 and all(a != b for a, b in zip(c, c[1:])) \
        and c[0] in (0, 7, 8) and c[-1] in (0, 7, 8)


def stats(text, oracle):
    """what a generated file holds, as the reference sees it: records, irregular records (RB_F_REGULAR clear after remove_trailing_indels)
    and those whose CIGAR the default configuration changes, deferred pairs per group in the first pass, contained records, groups whose
    largest overlap is tied, q_st = 0 records, _TO. lines, and the irregular records that pairs of two or more passes cut (the host driver
    on the oracle's kernels)"""
    from rustybam_amd import trim_driver
    recs = parse(text)
    n = len(recs)
    order = np.array(sorted(range(n), key=lambda i: recs[i]["q_name"]))
    names = [recs[i]["q_name"] for i in order]
    grp = np.cumsum(np.r_[0, [a != b for a, b in zip(names[1:], names[:-1])]]).astype(np.int64)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(r["cigar"]) for r in recs])
    col = lambda k: np.array([r[k] for r in recs], np.uint64)  # noqa: E731
    b = oracle.Batch(np.concatenate([r["cigar"] for r in recs]), off, col("t_st"), col("t_en"), col("q_st"), col("q_en"),
                     np.array([r["strand"] for r in recs], np.uint8))
    norm = oracle.normalize(b)
    irregular = np.array([not is_regular(r["cigar"][int(x["first_op"]):int(x["first_op"]) + int(x["n_ops"])]) for r, x in zip(recs, norm)])
    left, right, deferred, contained = trim_driver.select_pairs(order, grp, norm["q_st"].astype(np.uint64), norm["q_en"].astype(np.uint64))
    # per group: candidates (overlap >= 1, neither contained) and how many share the largest overlap
    qs, qe = norm["q_st"].astype(np.int64)[order], norm["q_en"].astype(np.int64)[order]
    per_group_deferred, tied = [], 0
    for g in range(int(grp[-1]) + 1 if n else 0):
        idx = np.flatnonzero(grp == g)
        ovs = []
        for a in range(len(idx)):
            for c in range(a + 1, len(idx)):
                i, j = idx[a], idx[c]
                ov = min(qe[i], qe[j]) - max(qs[i], qs[j])
                if ov >= 1 and ov != qe[j] - qs[j] and ov != qe[i] - qs[i]:
                    ovs.append(ov)
        per_group_deferred.append(max(0, len(ovs) - 1))
        tied += len(ovs) >= 2 and ovs.count(max(ovs)) >= 2
    # which records the passes cut (the host driver's bookkeeping on the oracle's kernels: indices are in name-sorted order)
    cuts = np.zeros(n, np.int64)

    class Log(OracleEngine):
        def overlap_split(self, *a, **k):
            for i in list(a[7]) + list(a[8]):
                cuts[int(i)] += 1
            return super().overlap_split(*a, **k)

    out = trim_driver.overlapping_paf_recs(Log(oracle), recs)
    rc, want = oracle.cli(*oracle_args("default"), stdin=text)
    changed = sum(1 for i, o in zip(order, out) if irregular[i] and not np.array_equal(recs[i]["cigar"], o["cigar"]))
    return dict(records=n, groups=len(per_group_deferred), irregular=int(irregular.sum()), irregular_cut=changed,
                irregular_cut_twice=int((irregular[order] & (cuts >= 2)).sum()), max_group=int(np.bincount(grp).max()),
                max_deferred_first_pass=max(per_group_deferred), deferred_first_pass=int(deferred), contained=int(contained.sum()),
                tied_groups=int(tied), q_st_zero=int(sum(r["q_st"] == 0 for r in recs)),
                q_st_zero_lead_no_query=int(sum(r["q_st"] == 0 and (int(r["cigar"][0]) & 15) not in QRY for r in recs)), to_lines=want.count(b"_TO."),
                oracle_rc=rc)
