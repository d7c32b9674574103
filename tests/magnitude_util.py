"""Inputs and references for the tests of the clip and pair kernels where 32 bits run out (tests/test_magnitude_inputs.py holds them to
the per-base oracle on the CPU, tests/test_gpu_magnitude.py holds the kernels to them).

Two kinds of input:
  * a small batch SHIFTED far out (shift): the per-base oracle keeps positions in u64 and costs memory per aligned unit, not per
    coordinate, so it still is the reference;
  * REGULAR records of 2^31 .. 2^32 - 1 units in a few dozen ops (spans_record, lane_record, tile_record_*) or a few hundred (tile_long_*:
    what reaches the tile kernel's span guards ON the tile kernel): 17 bytes a unit put them out of the per-base oracle's reach, so the
    reference is written here, in run-length form and exact integers: clip_regular / break_regular.

clip_regular restates trim_paf_rec_to_rgn (liftover.rs:17-105) on the arrays aligned_pairs would build (paf.rs:501-538) WITHOUT building
them: unit u of the alignment lies in op k at offset j, its t_pos / q_pos follow from the bases in front of op k, slice::binary_search
(both generations, as oracle/rb_oracle.c states them) probes that implicit array, the walk to a match base (paf.rs:547-561) is a walk
over ops.  Python ints only.  It is NOT a port of oracle/rb_opspace.c or of the kernels (which find a boundary's op from prefix sums in
closed form): those share the kernels' 32-bit assumptions, this has none."""
import bisect

import numpy as np

M, I, D, N, EQ, X = 0, 1, 2, 3, 7, 8
REF = frozenset((M, D, N, EQ, X))
QRY = frozenset((M, I, EQ, X))
MATCH = frozenset((M, EQ, X))
OPCH = "MIDNSHP=X"
OP_CAP = 1 << 28  # a packed op word holds lengths below this (include/rustybam_amd.h); longer ops take a continuation word and are not regular
MODERN, LEGACY = 0, 1
OK, NONE_INDEL, PANIC_NOTFOUND, PANIC_OVERFLOW = 0, 1, 16, 22

SHIFTS = ((2**32 - 1500, 2**32 - 1500), (2**32 + 12345, 2**33 + 7), (2**40 + 7, 2**52 + 3), (2**62, 2**62))


# ------------------------------------------------------------------ shifted inputs
def shift(b, w, Kt, Kq):
    """the batch b (and the windows w = (w_contig, w_st, w_en), or None) with Kt added to every target coordinate and Kq to every query
    coordinate; ops, offsets, strands and contigs are shared, not copied"""
    kt, kq = np.uint64(Kt), np.uint64(Kq)
    nb = dict(b)
    nb["t_st"], nb["t_en"] = b["t_st"].astype(np.uint64) + kt, b["t_en"].astype(np.uint64) + kt
    nb["q_st"], nb["q_en"] = b["q_st"].astype(np.uint64) + kq, b["q_en"].astype(np.uint64) + kq
    if w is None:
        return nb, None
    return nb, (w[0], w[1].astype(np.uint64) + kt, w[2].astype(np.uint64) + kt)


def shift_paf_text(text, Kt, Kq):
    """PAF text with Kq added to columns 3, 4 (query start, end) and 2 (query length), Kt to columns 8, 9 and 7"""
    out = []
    for ln in text.splitlines():
        t = ln.split("\t")
        for c, k in ((1, Kq), (2, Kq), (3, Kq), (6, Kt), (7, Kt), (8, Kt)):
            t[c] = str(int(t[c]) + k)
        out.append("\t".join(t))
    return "\n".join(out) + "\n"


def shift_bed_text(text, K):
    out = []
    for ln in text.splitlines():
        t = ln.split("\t")
        if len(t) >= 3 and t[1].isdigit() and t[2].isdigit():
            t[1], t[2] = str(int(t[1]) + K), str(int(t[2]) + K)
        out.append("\t".join(t))
    return "\n".join(out) + "\n"


# ------------------------------------------------------------------ the run-length reference
def as_ops(cigar):
    """'5=3I', packed words or (length, code) pairs -> [(length, code)] of Python ints"""
    if isinstance(cigar, str):
        out, n = [], 0
        for ch in cigar:
            if ch.isdigit():
                n = n * 10 + int(ch)
            else:
                out.append((n, OPCH.index(ch)))
                n = 0
        return out
    out = []
    for v in cigar:
        out.append((int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v) >> 4, int(v) & 15))
    return out


def pack_ops(ops):
    assert all(0 < ln < OP_CAP for ln, _ in ops)
    return [(ln << 4) | c for ln, c in ops]


def cigar_string(ops):
    return "".join(f"{ln}{OPCH[c]}" for ln, c in ops)


def is_regular(ops):
    """RB_F_REGULAR but for the size (include/rustybam_amd.h): M I D N = X only, every length >= 1 and in one word, no two neighbours of
    one type, a match op at both ends"""
    return bool(ops) and all(c in (M, I, D, N, EQ, X) and 1 <= ln < OP_CAP for ln, c in ops) and \
        all(a[1] != b[1] for a, b in zip(ops, ops[1:])) and ops[0][1] in MATCH and ops[-1][1] in MATCH


def sums(ops):
    """(sR, sQ, U): reference bases, query bases, aligned units"""
    return (sum(ln for ln, c in ops if c in REF), sum(ln for ln, c in ops if c in QRY), sum(ln for ln, _ in ops))


class _Aln:
    """the arrays of aligned_pairs (paf.rs:501-538) of a regular record, as functions of the unit index"""

    def __init__(self, ops, t_st, q_st, strand):
        assert is_regular(ops), "clip_regular / break_regular take regular records only"
        self.ops, self.t_st, self.q_st = ops, int(t_st), int(q_st)
        self.minus = strand in ("-", ord("-"), b"-")
        self.P, self.Rb, self.Qb = [0], [0], [0]  # units, reference bases, query bases in front of op k
        for ln, c in ops:
            self.P.append(self.P[-1] + ln)
            self.Rb.append(self.Rb[-1] + (ln if c in REF else 0))
            self.Qb.append(self.Qb[-1] + (ln if c in QRY else 0))
        self.U, self.t_en, self.q_en = self.P[-1], self.t_st + self.Rb[-1], self.q_st + self.Qb[-1]

    def op_of(self, u):
        k = bisect.bisect_right(self.P, u) - 1
        return k, u - self.P[k]

    def tpos(self, u):  # t_pos starts at t_st - 1 and steps before it is pushed (:505, :523-525, :532)
        k, j = self.op_of(u)
        return self.t_st + self.Rb[k] + (j if self.ops[k][1] in REF else -1)

    def qpos(self, u):  # '+': as t_pos; '-': starts at q_en and steps down (:512-514, :526-531)
        k, j = self.op_of(u)
        if self.ops[k][1] in QRY:
            return self.q_en - self.Qb[k] - j - 1 if self.minus else self.q_st + self.Qb[k] + j
        return self.q_en - self.Qb[k] if self.minus else self.q_st + self.Qb[k] - 1

    def search(self, key, policy):
        """tpos_aln.binary_search(&key) (paf.rs:541-544): the index it returns, None for Err.  The two generations of the standard
        library differ in which of several equal elements they find (a base and the insertion behind it share a t_pos)."""
        if policy == MODERN:  # rustc 1.82 on
            size, base = self.U, 0
            while size > 1:
                half = size // 2
                mid = base + half
                if self.tpos(mid) <= key:
                    base = mid
                size -= half
            return base if self.tpos(base) == key else None
        left, right = 0, self.U  # rustc 1.52 .. 1.81
        size = self.U
        while left < right:
            mid = left + size // 2
            v = self.tpos(mid)
            if v < key:
                left = mid + 1
            elif v > key:
                right = mid
            else:
                return mid
            size = right - left
        return None

    def to_match(self, u, right):
        """paf.rs:547-561: from unit u to the closest match base to the right (left)"""
        k, _ = self.op_of(u)
        if self.ops[k][1] in MATCH:
            return u
        if right:
            while k < len(self.ops) and self.ops[k][1] not in MATCH:
                k += 1
            return self.P[k]  # (a regular record ends on a match op: k stays inside)
        while k > 0 and self.ops[k][1] not in MATCH:
            k -= 1
        return self.P[k + 1] - 1 if self.ops[k][1] in MATCH else 0

    def subset(self, s, e):
        """subset_cigar + collapse_long_cigar (paf.rs:593-620) of units s ..= e"""
        (ks, js), (ke, je) = self.op_of(s), self.op_of(e)
        if ks == ke:
            return [(je - js + 1, self.ops[ks][1])]
        return [(self.ops[ks][0] - js, self.ops[ks][1])] + list(self.ops[ks + 1:ke]) + [(je + 1, self.ops[ke][1])]


def _clip(a, ws, we, policy):
    ws, we = int(ws), int(we)
    if not (a.t_en > ws and a.t_st < we):  # paf_overlaps_rgn, paf.rs:622-627
        return None
    if a.t_st > ws and a.t_en < we:  # liftover.rs:23-25: the record as it is, under its own id
        s, e, inside = 0, a.U - 1, True
    else:
        inside = False
        s = a.search(max(ws, a.t_st), policy)  # :28-35
        e = a.search(min(we, a.t_en) - 1, policy)  # :38-49
        if s is None or e is None:
            return dict(status=PANIC_NOTFOUND)
        s, e = a.to_match(s, True), a.to_match(e, False)
        if s > e:  # :52-54
            return dict(status=NONE_INDEL)
    ops = a.subset(s, e)  # (both ends are match bases: nothing for remove_trailing_indels, and a match op is there, :66-89)
    t0, t1, q0, q1 = a.tpos(s), a.tpos(e), a.qpos(s), a.qpos(e)  # :57-60
    if a.minus:  # :77-79
        q0, q1 = q1, q0
    R, Q, U = sums(ops)
    assert t1 + 1 - t0 == R and q1 + 1 - q0 == Q  # check_integrity, :99-102
    return dict(status=OK, inside=inside, t_st=t0, t_en=t1 + 1, q_st=q0, q_en=q1 + 1, nmatch=sum(ln for ln, c in ops if c in MATCH) & 0xFFFFFFFF,
                aln_len=U & 0xFFFFFFFF, ops=ops)


def clip_regular(cigar, t_st, q_st, strand, ws, we, policy=MODERN):
    """trim_paf_rec_to_rgn (liftover.rs:17-105) of a regular record and the window [ws, we): None where the two do not overlap, else a
    dict of status (0, or 1: the window holds no match base) and, for status 0, inside (the record as it is), t_st, t_en, q_st, q_en,
    nmatch, aln_len (as the u32 the rows hold) and ops = [(length, code)]"""
    return _clip(_Aln(as_ops(cigar), t_st, q_st, strand), ws, we, policy)


def break_regular(cigar, t_st, q_st, strand, max_size, policy=MODERN):
    """break_paf_on_indels (liftover.rs:182-226): the pieces between the indels longer than max_size become windows, the windows become
    clips.  -> [((st, en), clip)] in the reference's order, every candidate window with its clip's status"""
    a = _Aln(as_ops(cigar), t_st, q_st, strand)
    cur = pre = a.t_st
    windows = []
    for ln, c in a.ops:
        if ln > int(max_size) and c in (I, D):
            if cur > pre:
                windows.append((pre, cur))
            pre = cur + (ln if c in REF else 0)
        if c in REF:
            cur += ln
    if cur > pre:
        windows.append((pre, cur))
    return [(w, _clip(a, w[0], w[1], policy)) for w in windows]


def _rows(hits, n_ops_hint=0):
    """[(rec, win, clip)] -> (rows in the oracle's layout, out ops), as oracle.liftover / oracle.break_paf return them"""
    from oracle import pyoracle
    rows = np.zeros(len(hits), pyoracle.HIT_DT)
    out = []
    for i, (rec, win, c) in enumerate(hits):
        rows[i]["rec"], rows[i]["win"], rows[i]["status"] = rec, win, c["status"]
        if c["status"] != OK:
            rows[i]["out_off"] = len(out)
            continue
        for k in ("t_st", "t_en", "q_st", "q_en", "nmatch", "aln_len"):
            rows[i][k] = c[k]
        rows[i]["flags"] = 1 if c["inside"] else 0
        words = pack_ops(c["ops"])
        rows[i]["out_off"], rows[i]["out_n"] = len(out), len(words)
        out += words
    return rows, np.array(out, np.uint32)


def _records(b):
    off = [int(x) for x in b["op_off"]]
    for r in range(len(off) - 1):
        yield r, _Aln(as_ops(b["ops"][off[r]:off[r + 1]]), int(b["t_st"][r]), int(b["q_st"][r]), int(b["strand"][r]))


def liftover_regular(b, w, policy=MODERN):
    """oracle.liftover's rows for a batch of regular records, from clip_regular: contigs by first appearance, then record order, then
    window order (liftover.rs:151, oracle/rb_oracle.c rbo_liftover_arrays)"""
    wc, ws, we = ([int(x) for x in a] for a in w)
    contig = [int(x) for x in b["contig"]]
    rank = {}
    for c in contig:
        rank.setdefault(c, len(rank))
    recs = dict(_records(b))
    hits = []
    for r in sorted(recs, key=lambda r: (rank[contig[r]], r)):
        for g in range(len(ws)):
            if wc[g] != contig[r]:
                continue
            c = _clip(recs[r], ws[g], we[g], policy)
            if c is not None:
                hits.append((r, g, c))
    return _rows(hits)


def break_paf_regular(b, max_size, policy=MODERN):
    """oracle.break_paf's rows for a batch of regular records, from break_regular's pieces"""
    hits = []
    for r, a in _records(b):
        for p, (_, c) in enumerate(break_regular(a.ops, a.t_st, a.q_st, "-" if a.minus else "+", max_size, policy)):
            hits.append((r, p, c))
    return _rows(hits)


# ------------------------------------------------------------------ big regular records
def batch_of(records, contig=None):
    """[(ops, t_st, q_st, strand)] -> batch dict (the form rbtest_util.random_batch returns)"""
    words = [np.array(pack_ops(r[0]), np.uint32) for r in records]
    off = np.zeros(len(records) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in words])
    S = [sums(r[0]) for r in records]
    u = lambda v: np.array(v, np.uint64)  # noqa: E731
    return dict(ops=np.concatenate(words) if words else np.zeros(0, np.uint32), op_off=off,
                t_st=u([r[1] for r in records]), t_en=u([r[1] + s[0] for r, s in zip(records, S)]),
                q_st=u([r[2] for r in records]), q_en=u([r[2] + s[1] for r, s in zip(records, S)]),
                strand=np.array([ord(r[3]) for r in records], np.uint8),
                contig=np.zeros(len(records), np.uint32) if contig is None else np.array(contig, np.uint32))


def _codes(rng, n, need_all=True):
    """n op codes of a regular record: = / X alternating, some of the inner ones I, D or N instead (need_all: each of the three is there)"""
    while True:
        c = []
        for i in range(n):
            inner = 0 < i < n - 1
            while True:
                x = int(rng.choice([EQ, X, I, D, N], p=[.4, .25, .13, .13, .09])) if inner else int(rng.choice([EQ, X]))
                if not c or x != c[-1]:
                    break
            c.append(x)
        if not need_all or {I, D, N} <= set(c):
            return c


def small_regular(rng, n_rec, max_ops=14):
    """[(ops, t_st, q_st, strand)]: short regular records (N ops among them) of short ops, both strands, some at t_st = 0 / q_st = 0"""
    out = []
    for _ in range(n_rec):
        codes = _codes(rng, int(rng.integers(1, max_ops + 1)), need_all=False)
        ops = [(int(rng.choice([1, 2, 3, 9, 40], p=[.4, .2, .2, .15, .05])), c) for c in codes]
        out.append((ops, int(rng.choice([0, 1, 7, 2500])), int(rng.choice([0, 3, 1200])), "+-"[int(rng.integers(0, 2))]))
    return out


def edge_windows(rng, ops, t_st, n):
    """n windows [ws, we) for the record (ops, t_st) whose ends are drawn from: the record's first and last base, the bases around every op
    boundary (so: the base in front of an I, whose t_pos the insertion shares; the first, an inner and the last base of a D or N), bases
    inside ops, and positions around the record"""
    Rb = [0]
    for ln, c in ops:
        Rb.append(Rb[-1] + (ln if c in REF else 0))
    sR = Rb[-1]
    marks = {-3, -1, 0, 1, sR - 1, sR, sR + 1, sR + 4}
    for k, (ln, c) in enumerate(ops):
        marks |= {Rb[k] - 1, Rb[k], Rb[k] + 1, Rb[k] + ln // 2, Rb[k + 1] - 1}
    marks = sorted(m for m in marks if t_st + m >= 0)
    out = []
    while len(out) < n:
        a, b = int(rng.choice(marks)), int(rng.choice(marks))
        if a > b:
            a, b = b, a
        out.append((t_st + a, t_st + b + 1))  # (never empty)
    return out


SPAN_SIZES = (2**31 - 1, 2**31, 2**31 + 1, 3_000_000_019, 2**32 - 1)
_SPAN_OPS = {2**31 - 1: 15, 2**31: 24, 2**31 + 1: 33, 3_000_000_019: 37, 2**32 - 1: 40, 2**32: 40}


def spans_record(U, seed=0):
    """a regular record of exactly U units in 15 .. 40 ops, each below 2^28: a fifth of the ops short (1 .. 150), the others share the rest"""
    rng = np.random.default_rng((int(U) * 31 + seed) & 0xFFFFFFFF)
    n = _SPAN_OPS[U]
    codes = _codes(rng, n)
    small = set(int(x) for x in rng.choice(np.arange(1, n - 1), n // 5, replace=False))
    ln = [int(rng.integers(1, 151)) if i in small else 0 for i in range(n)]
    big = [i for i in range(n) if i not in small]
    wts = [float(x) for x in rng.uniform(0.8, 1.0, len(big))]
    rest = U - sum(ln)
    for i, wt in zip(big, wts):
        ln[i] = int(rest * wt / sum(wts))
    ln[big[0]] += U - sum(ln)
    ops = list(zip(ln, codes))
    assert is_regular(ops) and sums(ops)[2] == U
    return ops


def span_windows(ops, t_st):
    """windows (sorted by start) for a spans record at t_st: one base wide at reference offsets 0, 2^31 - 1, 2^31, 2^31 + 1 and sR - 1 and at
    the reference positions of units 2^31 - 1, 2^31, 2^31 + 1 (where the record reaches them); windows that cut inside the ops around
    those places; one that ends inside a D; the whole record, exactly and with room around it"""
    a = _Aln(ops, t_st, 0, "+")
    sR = a.Rb[-1]
    w = {(t_st, t_st + 1), (t_st + sR - 1, t_st + sR), (t_st, t_st + sR), (max(t_st, 5) - 5, t_st + sR + 5), (t_st + sR // 3, t_st + sR // 3 + 12345)}
    marks = [2**31 - 1, 2**31, 2**31 + 1]
    marks += [a.tpos(u) - t_st for u in (2**31 - 1, 2**31, 2**31 + 1) if u < a.U]
    for o in marks:
        if 0 <= o < sR:
            w.add((t_st + o, t_st + o + 1))
            w.add((t_st + max(o - 1000, 0), t_st + min(o + 1000, sR)))  # cuts inside the ops around it
            k = bisect.bisect_right(a.Rb, o) - 1  # the op that holds this base: from inside it to inside the next but one
            hi = a.Rb[min(k + 3, len(ops))]
            w.add((t_st + o, t_st + min(hi - 1, sR)))
    for k, (ln, c) in enumerate(ops):
        if c == D:  # from inside the op in front of a D to inside the D; from inside the D on
            w.add((t_st + max(a.Rb[k] - 7, 0), t_st + a.Rb[k] + (ln + 1) // 2))
            w.add((t_st + a.Rb[k] + ln // 2, t_st + min(a.Rb[k + 1] + 9, sR)))
            w.add((t_st + a.Rb[k], t_st + a.Rb[k + 1]))  # the D alone: no match base
    w = sorted(x for x in w if x[1] > x[0])
    return (np.zeros(len(w), np.uint32), np.array([x[0] for x in w], np.uint64), np.array([x[1] for x in w], np.uint64))


def lane_sums(b, r):
    """the sums of lengths the lanes of the stream kernel see of record r: a lane holds 8 ops, and the 512-op steps start at the batch's op
    offset rounded down to a multiple of 32 (rb_stream.h: head = rec0 & 31) -- at the record's first op where that offset is one"""
    o0, o1 = int(b["op_off"][r]), int(b["op_off"][r + 1])
    head = o0 & 31
    out = {}
    for i in range(o1 - o0):
        out[(head + i) // 8] = out.get((head + i) // 8, 0) + (int(b["ops"][o0 + i]) >> 4)
    return [out.get(k, 0) for k in range(max(out) + 1)]


LANE_SUMS = (2**25 - 1, 2**25, 2**25 + 1)


def lane_record(total, first):
    """a 64-op regular record whose ops first .. first + 7 sum to `total`, every other op short"""
    rng = np.random.default_rng(total % 1000 + first)
    codes = [(EQ, X)[i % 2] for i in range(64)]
    for k, i in enumerate((5, 9, 14, 21, 30, 47)):  # indels and introns, among them ops of the eight
        codes[i] = (I, D, N)[k % 3]
    ln = [int(rng.integers(1, 40)) for _ in range(64)]
    each = total // 8
    for i in range(first, first + 8):
        ln[i] = each
    ln[first + 3] += total - 8 * each
    ops = list(zip(ln, codes))
    assert is_regular(ops) and sum(ln[first:first + 8]) == total
    return ops


# ---- the tile kernel's guards (k_tile.hip: sR < 2^31 and sQ < 2^31 per record, the tile's sum of sR + sQ below 2^32)
def _fill(codes, big, total, small=3):
    """lengths for `codes`: the ops at `big` share what is left of `total` units of THEIR kind, the others are `small`"""
    ln = [small] * len(codes)
    each = total // len(big)
    for i in big:
        ln[i] = each
    ln[big[-1]] += total - each * len(big)
    assert all(0 < x < OP_CAP for x in ln), ln
    return list(zip(ln, codes))


TILE_SMALL = [(5, EQ), (2, X), (3, I), (7, EQ), (4, D), (9, EQ), (1, X), (2, N), (6, EQ), (3, X)]  # a short record to share a tile with


def tile_record_sR(sR):
    """11 ops, sR reference bases exactly, a handful of query bases: D and N ops hold the reference"""
    codes = [EQ, D, N, D, N, D, N, D, N, D, X]
    big = [1, 2, 3, 4, 5, 6, 7, 8, 9]
    ops = _fill(codes, big, sR - 2 * 3)
    assert sums(ops)[0] == sR and is_regular(ops)
    return ops


def tile_record_sQ(sQ):
    """17 ops (eight I ops below 2^28 each need seven ops between them and a match op at either end), sQ query bases exactly, few reference bases"""
    codes = [EQ, I, X, I, D, I, X, I, EQ, I, X, I, D, I, X, I, EQ]
    big = [1, 3, 5, 7, 9, 11, 13, 15]
    small_q = 40 * sum(1 for i, c in enumerate(codes) if i not in big and c in QRY)  # (40: eight I ops of 2^31 / 8 - 35 stay in one word)
    ops = _fill(codes, big, sQ - small_q, small=40)
    assert sums(ops)[1] == sQ and is_regular(ops)
    return ops


def tile_total_records(tot):
    """four records of 9 .. 12 ops whose sR + sQ sum to `tot`: three that hold nearly 2^31 / 3 reference bases each in D and N ops (so the
    last record starts near 2^31 in the tile's running reference total) and one of long = ops, about 2^30 bases of either kind, sized to
    land on tot"""
    recs, used = [], 0
    for j, codes in enumerate(([EQ, D, X, N, EQ, D, X, N, EQ], [EQ, D, X, N, EQ, D, X, N, EQ, X], [EQ, D, X, N, EQ, D, X, N, EQ, D, X])):
        ops = _fill(codes, [i for i, c in enumerate(codes) if c in (D, N)], 715_827_000 + j)
        recs.append(ops)
        used += sums(ops)[0] + sums(ops)[1]
    rest = tot - used
    codes = [EQ, X, EQ, I, EQ, X, EQ, D, EQ, X, EQ, X]
    small_bases = 3 * (4 * 2 + 1 + 1)  # the short ops: four X (a base of either kind per unit), an I, a D
    ops = _fill(codes, [0, 2, 4, 6, 8, 10], (rest - small_bases) // 2)
    if (rest - small_bases) % 2:  # an odd rest: one more query base, on the I
        ops[3] = (ops[3][0] + 1, I)
    recs.append(ops)
    assert sum(sums(o)[0] + sums(o)[1] for o in recs) == tot and all(is_regular(o) and 9 <= len(o) <= 12 for o in recs)
    return recs


# The tile kernel also hands a tile back when the eight ops of one of its lanes sum to 2^25 or more (k_tile.hip: v_maxsu), which records of a
# dozen ops this large always do.  To reach its span guards ON the tile kernel a record needs 2^31 bases in lanes that stay below 2^25:
# several hundred ops, long and short ones in turn, so that any eight neighbours hold four long ones.
def _striped(n, big_at_odd, big_codes, small_codes, total):
    """n ops (odd): the ops at odd (or even) places are long and share `total` units, the others are 1 .. 3 units"""
    codes, ln, big = [], [], []
    for i in range(n):
        is_big = (i % 2 == 1) == big_at_odd
        src = big_codes if is_big else small_codes
        codes.append(src[(i // 2) % len(src)])
        ln.append(0 if is_big else 1 + i % 3)
        if is_big:
            big.append(i)
    each = total // len(big)
    for i in big:
        ln[i] = each
    ln[big[-1]] += total - each * len(big)
    ops = list(zip(ln, codes))
    assert is_regular(ops), "striped record"
    return ops


def _ref_small(n):  # reference (= query) bases of the short match ops of a striped record whose long ops sit at the odd places
    return sum(1 + i % 3 for i in range(0, n, 2))


def tile_long_sR(sR, n=561):
    ops = _striped(n, True, (D, N), (EQ, X), sR - _ref_small(n))
    assert sums(ops)[0] == sR
    return ops


def tile_long_sQ(sQ, n=561):
    ops = _striped(n, True, (I,), (EQ, X), sQ - _ref_small(n))
    assert sums(ops)[1] == sQ
    return ops


def tile_long_total(tot):
    """as tile_total_records, in records of 201, 201, 201 and 301 ops whose lanes stay below 2^25"""
    recs = [tile_long_sR(715_827_000 + j, 201) for j in range(3)]
    rest = tot - sum(sums(o)[0] + sums(o)[1] for o in recs)
    n = 301
    small = sum(1 + i % 3 for i in range(1, n, 2))  # the short X ops, a base of either kind per unit ...
    l1 = 2 - rest % 2                               # ... but op 1 (2 units in the stripe), an insertion of 1 or 2 bases: the parity of the rest
    ops = _striped(n, False, (EQ,), (X,), (rest - 2 * (small - 2) - l1) // 2)
    ops[1] = (l1, I)
    recs.append(ops)
    assert sum(sums(o)[0] + sums(o)[1] for o in recs) == tot and all(is_regular(o) for o in recs)
    return recs


def max_lane_sum(b):
    """the largest sum of eight neighbouring op lengths at any alignment, over the whole batch (what a lane of the tile kernel can hold)"""
    ln = [int(v) >> 4 for v in b["ops"]]
    return max(sum(ln[i:i + 8]) for i in range(max(1, len(ln) - 7)))


def tile_batch(recs, strands="+-+-"):
    """the records one behind the other on one contig, 1000 bases apart"""
    out, t = [], 1000
    for j, ops in enumerate(recs):
        out.append((ops, t, 500 + 7 * j, strands[j % len(strands)]))
        t += sums(ops)[0] + 1000
    return batch_of(out)


def last_record_windows(b):
    """window lists on the batch's last record only, each with starts and ends that do not decrease (what the tile kernel takes): its first
    and last base, cuts inside its ops, its halves; and, lists of their own, all of it exactly and with room around it"""
    r = len(b["t_st"]) - 1
    t0, t1 = int(b["t_st"][r]), int(b["t_en"][r])
    sR = t1 - t0
    lists = [[(t0 - 5, t0 + 1), (t0, t0 + 1), (t0, t0 + 2), (t0 + 1, t0 + sR // 2), (t0 + sR // 4, t0 + sR // 2 + 1), (t0 + sR // 2 - 3, t1 - 2),
              (t0 + sR // 2, t1 - 1), (t1 - 1, t1), (t1 - 1, t1 + 100)], [(t0, t1)], [(t0 - 5, t1 + 100)]]
    return [(np.zeros(len(w), np.uint32), np.array([x[0] for x in w], np.uint64), np.array([x[1] for x in w], np.uint64)) for w in lists]


# ------------------------------------------------------------------ the pair row kernel's score guard
def guard_pairs(total):
    """pairs of short regular records whose query spans sum to `total` (k_trim4.hip: smax * (Lq + Rq) >= 2^29 leaves the row kernel): every
    combination of strands, overlaps of a few dozen bases, a few indels in the overlap"""
    recs, left, right = [], [], []
    for k, (sa, sb) in enumerate((a, b) for a in "+-" for b in "+-"):
        qa = total // 2 - 6 + 3 * k
        qb = total - qa
        ops_a = [(qa - 60, EQ), (4, D), (20, X), (2, I), (30, EQ), (3, D), (8, EQ)]
        ops_b = [(11, EQ), (3, I), (17, X), (5, D), (qb - 31 - 40, EQ), (1, X), (39, EQ)]
        assert sums(ops_a)[1] == qa and sums(ops_b)[1] == qb
        ov = 37 + 5 * k
        a0 = 100 + 1000 * k
        recs.append((ops_a, 5000 + k, a0, sa))
        recs.append((ops_b, 9000 + k, a0 + qa - ov, sb))
        left.append(2 * k); right.append(2 * k + 1)
    b = batch_of(recs)
    del b["contig"]
    return b, np.array(left, np.uint32), np.array(right, np.uint32)


def wide_pair():
    """one pair with an overlap of 1500 bases: at a score of 2^20 the sums reach 1.6e9, inside i32 and far above the row kernel's guard"""
    ops_a = [(700, EQ), (3, X), (900, EQ), (2, I), (400, EQ), (4, D), (300, X), (1, I), (200, EQ)]
    ops_b = [(500, EQ), (2, D), (333, X), (5, I), (900, EQ), (1, X), (700, EQ)]
    qa = sums(ops_a)[1]
    b = batch_of([(ops_a, 100, 50, "+"), (ops_b, 7000, 50 + qa - 1500, "-")])
    del b["contig"]
    return b, np.array([0], np.uint32), np.array([1], np.uint32)


# ------------------------------------------------------------------ a trim-paf file of regular records
def trim_groups_text(seed, n_rec=2000, lo=40, hi=121):
    """PAF text: n_rec regular records of lo .. hi - 1 ops, four to a query whose neighbouring spans overlap by 5 .. 59 bases (nothing
    contained), both strands: every pair is one the in-place pair kernels cut where it lies"""
    rng = np.random.default_rng(seed)
    lines = []
    for g in range(n_rec // 4):
        q0 = int(rng.integers(0, 3000))
        for j in range(4):
            n = int(rng.integers(lo, hi)) | 1  # match ops (= X M) at the even places, I and D between them
            code = np.where(np.arange(n) % 2 == 0, rng.choice([EQ, X, M], n, p=[.7, .2, .1]), rng.choice([I, D], n))
            ln = rng.choice([1, 2, 3, 9, 150], n, p=[.45, .2, .15, .15, .05])
            ops = [(int(a), int(c)) for a, c in zip(ln, code)]
            R, Q, _ = sums(ops)
            ts = int(rng.integers(0, 100_000))
            lines.append(f"q{g}\t20000\t{q0}\t{q0 + Q}\t{'+-'[int(rng.integers(0, 2))]}\tt{g % 3}\t200000\t{ts}\t{ts + R}\t{R}\t{max(R, Q)}\t60\tcg:Z:{cigar_string(ops)}")
            q0 += Q - int(rng.integers(5, 60))
    order = rng.permutation(len(lines))  # (the reference sorts by query name, stably)
    return "\n".join(lines[i] for i in order) + "\n"
