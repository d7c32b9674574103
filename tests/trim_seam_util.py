"""Planted inputs for the trim-paf pair kernels (k_trim4.hip, k_trim.hip, rb_pair.h) and a numpy restatement of where each attempt of
rb_dev_overlap_split's cascade puts a record's region.

The cascade: the row form with a region of 16 T ops at one end of the record (T = 4, then T = 8), the wave form with the ops around the
overlap staged (at most 192, 1024, 6144 ops in LDS, 32768 in a device slab), the serial kernel.  Whether an attempt takes a pair is a
matter of a few sizes: the record's length n, the ops ia / ib that hold the overlap's first / last base in the record's op order, and the
query offsets xa / xb of those bases.  The functions below restate those decisions; tests/test_trim_seam_inputs.py proves on the CPU that
every planted case sits where its name says, tests/test_gpu_trim_seams.py compares the kernels with the oracle on them and then checks
the route the diagnostic word of the row reports.

Geometry.  The overlap of a pair is [max q_st, min q_en) on the query.  For two records neither of which contains the other it is one END
of each record in op order: the left record's tail on '+' and its head on '-', the right record's head on '+' and its tail on '-'.  A
planted record therefore names the end (`tail` / `head`) and the op `far` that holds the overlap's other end; the strand follows from the
side the record is put on.  The partner is a short record of long ops that every attempt stages whole."""
import zlib

import numpy as np

from trim_util import is_regular

M, I, D, N, EQ, X = 0, 1, 2, 3, 7, 8
QRY_CODES, MATCH_CODES = (M, I, EQ, X), (M, EQ, X)
ROW_T = (4, 8)                         # the row form's two attempts: regions of 16 T ops
WAVE_CAPS = (192, 1024, 6144, 32768)   # the wave form's four (RB_TW_CAP .. RB_TW_CAP3)
STEP, MARGIN_START, MARGIN_END = 64, 16, 17
SLABS, WALK = 48, 64                   # the slab attempt: 48 workgroups, 64 list entries per workgroup and round
SCORES = ((1, 1, 1), (2, 3, 5))
MODERN, LEGACY = 0, 1
ST_OK = 0


def words(ops):
    """[(code, length), ...] -> packed words"""
    return np.array([(int(ln) << 4) | int(c) for c, ln in ops], np.uint32)


def record(ops):
    """a regular record from an explicit op list: only = X M I D N, every length >= 1, no two neighbours of one type, a match op at both ends"""
    w = words(ops) if not isinstance(ops, np.ndarray) else ops
    if not is_regular(w):
        raise ValueError(f"not a regular record: {ops[:8]}..")
    return w


def body(n, seed, fixed=None, maxlen=3):
    """a regular record of n ops with lengths 1 .. maxlen (the ends: 2, so that a clip that asks for the record's first base outside its region
    is answered); `fixed` = {index: (code, length)} plants ops.  Ops that are not planted never form a D / N run of two ops: every decline
    that depends on such a run is planted."""
    rng = np.random.default_rng(zlib.crc32(f"{seed}/{n}".encode()))
    fixed = fixed or {}
    out = []
    for i in range(n):
        if i in fixed:
            out.append(fixed[i])
            continue
        prev = out[-1][0] if out else None
        nxt = fixed.get(i + 1, (None, 0))[0]
        if i == 0 or i == n - 1:
            pool = [EQ, X, M]
        elif prev in (D, N) or nxt in (D, N) or i - 1 in fixed:  # (no D behind a planted op either: its last base keeps its own score)
            pool = [EQ, EQ, X, M, I]
        else:
            pool = [EQ, EQ, EQ, X, X, M, I, D]
        pool = [c for c in pool if c != prev and c != nxt]
        c = int(pool[int(rng.integers(0, len(pool)))])
        out.append((c, 2 if i in (0, n - 1) else int(rng.integers(1, maxlen + 1))))
    return record(out)


def qpre(w):
    """exclusive prefix of the query bases, n + 1 entries"""
    return np.concatenate([[0], np.cumsum(np.where(np.isin(w & 15, QRY_CODES), w >> 4, 0))]).astype(np.int64)


def op_of(w, x):
    """the query op that holds query offset x (op order); n: none"""
    return int(np.searchsorted(qpre(w), x, side="right")) - 1


def overlap_ends(w, left, minus, o):
    """(xa, xb, ia, ib) of an overlap of o bases at the record's end: rb_pair_open's offsets and the ops that hold them"""
    q = int(qpre(w)[-1])
    tail = left != minus
    xa, xb = (q - o, q - 1) if tail else (0, o - 1)
    return xa, xb, op_of(w, xa), op_of(w, xb)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def row_region(n, T, xa, xb, qtot):
    """(from_end, i0, m): the row form's region (k_trim4.hip, place)"""
    from_end = n > 16 * T and xa > qtot - 1 - min(xb, qtot - 1)
    m = min(n, 16 * T)
    return from_end, (n - m if from_end else 0), m


def row_decline(w, T, xa, xb, legacy):
    """why the row form with regions of 16 T ops leaves a pair with this record to the attempts behind it, as far as the record's sizes and
    op types say: 3 = a lane chunk of T ops without a query op, 'multi' = (legacy policy) a D / N run of two ops in the region, 4 = an
    overlap end outside the region, 7 = the op that holds xb is the region's last query op and the record goes on behind the region;
    0 = nothing.  (The order is the kernel's: the build of both records, the four searches, the run behind the last base.)"""
    n, p = len(w), qpre(w)
    _, i0, m = row_region(n, T, xa, xb, int(p[-1]))
    isq = np.isin(w[i0:i0 + m] & 15, QRY_CODES)
    full = np.concatenate([isq, np.ones(16 * T - m + 2, bool)])          # behind the region: zero-length M, a query op
    if (~full[:16 * T].reshape(16, T)).all(axis=1).any():
        return 3
    if legacy and (full[:-2] & ~full[1:-1] & ~full[2:])[:m].any():
        return "multi"
    ia, ib = op_of(w, xa), op_of(w, xb)
    if not (i0 <= ia < i0 + m and i0 <= ib < i0 + m):
        return 4
    lastq = i0 + int(np.flatnonzero(isq)[-1])
    if ib >= lastq and i0 + m < n:
        return 7
    return 0


def wave_region(n, cap, ia, ib):
    """[i0, i1) as rb_tw_stage (k_trim.hip) computes it: steps are multiples of 64 ops from op 0; the region starts 16 ops before the op that
    holds xa, or at the step before when that op is in lanes 0 .. 15 of its step (at op 0 in the record's first step); it ends 17 ops behind
    the op that holds xb, capped at n.  A record of at most `cap` ops is staged whole.  Forwards and backwards give the same region."""
    if n <= cap:
        return 0, n
    c0 = ia // STEP * STEP
    i0 = ia - MARGIN_START if ia - c0 >= MARGIN_START else max(c0 - STEP, 0)
    return i0, min(ib + MARGIN_END, n)


def wave_fits(n, cap, ia, ib):
    i0, i1 = wave_region(n, cap, ia, ib)
    return i1 - i0 <= cap


def predict(recs, legacy):
    """recs: (w, xa, xb) of the left and the right record -> (route, reasons): 'row' / 'wave' / 'serial' as the cascade's order gives it
    from the sizes alone, and the set of decline reasons met on the way ((T, reason) and ('wave', cap))"""
    reasons = set()
    for T in ROW_T:
        why = [row_decline(w, T, xa, xb, legacy) for w, xa, xb in recs]
        first = next((x for k in (3, "multi", 4, 7) for x in why if x == k), 0)
        if not first:
            return "row", reasons
        reasons.add((T, first))
    for cap in WAVE_CAPS:
        if all(wave_fits(len(w), cap, op_of(w, xa), op_of(w, xb)) for w, xa, xb in recs):
            return "wave", reasons
        reasons.add(("wave", cap))
    return "serial", reasons


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def partner(o, seed, head):
    """a short regular record of more than o query bases (a dozen ops, long = ops between single X I D M bases): every attempt stages it
    whole.  Its overlap is at its op-order head (`head`) or tail, and the op at that end -- the one under the planted record's far op -- is
    an X of b >= 2 bases where the planted far op is an =: the partner's overlapped bases score above 0 in sum, f rises over the overlap's
    first base (or falls over its last), so the split never lands on the overlap's far end and the clip never asks for the op in front of
    the far op, which a region that starts there cannot answer."""
    rng = np.random.default_rng(zlib.crc32(f"partner{seed}".encode()))
    e = o // 5 + 3
    ops, q = [(X, 2 + min(o // 16, 30))], 0
    while q < o + e + 5:
        ops.append((EQ, e + int(rng.integers(0, 3))))
        ops.append((int(rng.choice([X, I, D, M])), 1))
        q += ops[-2][1] + (ops[-1][0] != D)
    ops.append((EQ, e))
    assert len(ops) <= 64
    return record(ops if head else ops[::-1])


class Case:
    """one batch of pairs; every pair has records of its own.  route_open: why no route is expected (None: the restatement's route is)"""

    def __init__(self, name, item, scores=SCORES, policies=(MODERN, LEGACY), route_open=None, status=ST_OK, in_place=False):
        self.name, self.item, self.scores, self.policies, self.route_open, self.status, self.in_place = name, item, scores, policies, route_open, status, in_place
        self.cigs, self.q_st, self.strand, self.left, self.right, self.notes = [], [], [], [], [], []
        self._b = None

    def add_pair(self, lw, rw, sl, sr, o=None, b0=None, note=""):
        """the left record at a0, the right one so that the two overlap by o bases (or at b0 - a0 behind the left one's start)"""
        ql, qr = int(qpre(lw)[-1]), int(qpre(rw)[-1])
        a0 = 1000 + 11 * len(self.left)
        if b0 is None:
            if not 0 < o < min(ql, qr):
                raise ValueError(f"{self.name}: an overlap of {o} bases does not fit records of {ql} and {qr}")
            b0 = ql - o
        for w, q0, s in ((lw, a0, sl), (rw, a0 + b0, sr)):
            self.cigs.append(w); self.q_st.append(q0); self.strand.append(ord(s))
        self.left.append(len(self.cigs) - 2); self.right.append(len(self.cigs) - 1)
        self.notes.append(note)
        self._b = None

    def plant(self, w, end, far, j=0, seed=0, note=""):
        """four pairs: the record w as the left and as the right record of a pair, its overlap at its `end` ('tail' / 'head' in op order) with
        the overlap's other end in base j of op `far`; the partner on either strand.  The record's own strand follows from side and end."""
        p = qpre(w)
        if not (0 <= far < len(w) and (int(w[far]) & 15) == EQ and j < (int(w[far]) >> 4)):
            raise ValueError(f"{self.name}: op {far} cannot hold an overlap end (an = op: see partner)")
        o = int(p[-1] - (p[far] + j)) if end == "tail" else int(p[far] + j + 1)
        for left in (True, False):
            minus = (end == "tail") != left
            for ps in "+-":
                pw = partner(o, f"{self.name}{seed}{far}{ps}", head=left == (ps == "+"))  # (the partner is on the other side: its tail = !left != minus)
                s = "-" if minus else "+"
                if left:
                    self.add_pair(w, pw, s, ps, o, note=note)
                else:
                    self.add_pair(pw, w, ps, s, o, note=note)
                xa, xb, ia, ib = overlap_ends(w, left, minus, o)
                if (ib if end == "head" else ia) != far or (ia if end == "head" else ib) != (0 if end == "head" else len(w) - 1):
                    raise ValueError(f"{self.name}: the overlap of {o} bases ends in ops {ia}, {ib}, not in op {far}")

    def batch(self):
        if self._b is None:
            off = np.zeros(len(self.cigs) + 1, np.uint64)
            off[1:] = np.cumsum([len(c) for c in self.cigs])
            q_st = np.array(self.q_st, np.uint64)
            t_st = np.array([5000 + 3 * i for i in range(len(self.cigs))], np.uint64)
            code = [c & 15 for c in self.cigs]
            q = np.array([int(np.where(np.isin(k, QRY_CODES), c >> 4, 0).sum()) for c, k in zip(self.cigs, code)], np.uint64)
            r = np.array([int(np.where(np.isin(k, (M, D, N, EQ, X)), c >> 4, 0).sum()) for c, k in zip(self.cigs, code)], np.uint64)
            self._b = dict(ops=np.concatenate(self.cigs), op_off=off, t_st=t_st, t_en=t_st + r, q_st=q_st, q_en=q_st + q,
                           strand=np.array(self.strand, np.uint8))
        return self._b, np.array(self.left, np.uint32), np.array(self.right, np.uint32)

    def args(self):
        b, left, right = self.batch()
        return (b["ops"], b["op_off"], b["t_st"], b["t_en"], b["q_st"], b["q_en"], b["strand"]), left, right

    def geometry(self, i):
        """the pair's two records as predict() takes them: (w, xa, xb) from rb_pair_open's formulas; None where the spans do not overlap"""
        b, left, right = self.batch()
        rl, rr = int(left[i]), int(right[i])
        st, en = max(int(b["q_st"][rl]), int(b["q_st"][rr])), min(int(b["q_en"][rl]), int(b["q_en"][rr]))
        if en <= st:
            return None
        out = []
        for r in (rl, rr):
            qs, qe, minus = int(b["q_st"][r]), int(b["q_en"][r]), b["strand"][r] == ord("-")
            out.append((self.cigs[r], qe - en if minus else st - qs, qe - 1 - st if minus else en - 1 - qs))
        return out

    def routes(self, legacy):
        """per pair: (route, reasons) of the restatement"""
        out = []
        for i in range(len(self.left)):
            g = self.geometry(i)
            out.append(predict(g, legacy) if g else ("serial", {("open", 2)}))
        return out


def _plant_all(c, w, ends, far_of, **kw):
    for end in ends:
        c.plant(w, end, far_of(end, len(w)), **kw)


def case_row_length():
    """item 1: records of 63, 64, 65 and 127, 128, 129 ops, the overlap (a dozen ops) at either end"""
    c = Case("row_length", 1, in_place=True)
    for n in (63, 64, 65, 127, 128, 129):
        for end in ("tail", "head"):
            far = n - 13 if end == "tail" else 12
            c.plant(body(n, "rowlen", {far: (EQ, 2)}), end, far, j=1, note=f"n={n} {end}")
    return c


def case_row_edge():
    """item 2: the overlap's far end in region op 0, op 1 and one op outside the region (decline 4) of the from-end regions of a 200-op record
    ([136, 200) and [72, 200)); in the from-start regions the op that holds xb is the region's last query op (decline 7), with a query op and
    with a D as the region's last word, and one op further (decline 4)"""
    c = Case("row_edge", 2)
    for far in (136, 137, 135, 72, 73, 71):
        c.plant(body(200, f"edge{far}", {far: (EQ, 2)}), "tail", far, note=f"tail far={far}")
    for far, fx in ((63, {}), (62, {63: (D, 2)}), (62, {63: (I, 1)}), (64, {}), (127, {}), (126, {127: (D, 3)})):
        c.plant(body(200, f"edge{far}{sorted(fx)}", {far: (EQ, 2), **fx}), "head", far, j=1, seed=len(fx), note=f"head far={far} {fx}")
    return c


def case_row_chunks():
    """item 3: D / N runs against the row form's lane chunks (lane j owns ops [i0 + j T, i0 + (j + 1) T))"""
    c = Case("row_chunks", 3)
    run = lambda at, k: {at + e: ((D, N)[e & 1], 1 + (e & 1)) for e in range(k)}  # noqa: E731
    c.plant(body(200, "c4", {140: (EQ, 2), 147: (EQ, 2), **run(148, 4)}), "tail", 140, note="D N D N in lane 3 of [136, 200)")
    c.plant(body(200, "c4s", {140: (EQ, 2), 148: (X, 2), **run(149, 4)}), "tail", 140, note="the same one op on")
    c.plant(body(200, "c8", {120: (EQ, 2), 135: (EQ, 3), **run(136, 8)}), "tail", 120, note="D N x 4 in lane 8 of [72, 200)")
    c.plant(body(40, "dn", {20: (EQ, 2), 21: (D, 1), 22: (N, 2)}), "head", 20, j=1, note="D N behind the overlap's last base")
    for far in (139, 137):
        c.plant(body(200, "lane", {137: (EQ, 2), 139: (EQ, 2), 140: (D, 2)}), "tail", far, j=1, note=f"D in the next lane, far={far}")
    return c


def case_wave_length():
    """item 4: records of CAP and CAP + 1 ops.  (An overlap of two records that do not contain one another always reaches one end of each:
    what keeps the row forms away is an overlap that SPANS more than 128 ops, here 140.)"""
    c = Case("wave_length", 4, in_place=True)
    for cap in WAVE_CAPS[:3]:
        for n in (cap, cap + 1):
            for end in ("tail", "head"):
                far = n - 141 if end == "tail" else 140
                c.plant(body(n, "wlen", {far: (EQ, 2)}, maxlen=2), end, far, note=f"n={n} {end}")
    return c


def fit_far(cap, n, end, over):
    """the op that makes i1 - i0 == cap + over"""
    far = n - (cap + over) + MARGIN_START if end == "tail" else cap + over - MARGIN_END
    assert end == "head" or far % STEP >= MARGIN_START
    return far


def case_wave_fit(cap):
    """item 5: regions of exactly CAP and CAP + 1 ops"""
    c = Case(f"wave_fit_{cap}", 5)
    n = cap + 176 + (20 - (176 + MARGIN_START) % STEP) % STEP if cap != 32768 else 33100
    for end in ("tail", "head"):
        for over in (0, 1):
            far = fit_far(cap, n, end, over)
            c.plant(body(n, f"fit{end}{over}", {far: (EQ, 2)}, maxlen=2), end, far, note=f"{end} region {cap + over}")
    return c


def case_wave_steps():
    """item 6: where the ops that hold xa and xb lie inside their 64-op steps"""
    c = Case("wave_steps", 6, in_place=True)
    for far in (15, 16, 207, 208):
        c.plant(body(400, f"xa{far}", {far: (EQ, 2)}), "tail", far, j=1, note=f"xa in lane {far % 64} of step {far // 64}")
    for far in (174, 175, 191):
        c.plant(body(500, f"xb{far}", {far: (EQ, 2)}), "head", far, note=f"xb in lane {far % 64}")
    c.plant(body(260, "last", {258: (EQ, 1)}), "head", 258, note="xb in the op before the last: i1 = n")
    for n in (320, 321):
        c.plant(body(n, "walk", {n - 150: (EQ, 2)}), "tail", n - 150, note=f"n={n}: the backward walk's first step")
    c.plant(body(1100, "c0", {10: (EQ, 2)}), "tail", 10, note="a backward walk that reaches step 0 and does not fit below 6144")
    return c


def case_wave_direction():
    """item 6, the forwards / backwards choice: xa == Qtot - 1 - xb needs an overlap that touches neither end of the record, i.e. a right
    record inside the left one (the driver never sends such a pair; the kernels take it, and the oracle says what the reference does).  The
    left record's first op is long, so that a backward walk ends in the record's first step with the region still fitting 192 ops."""
    c = Case("wave_direction", 6, route_open="contained spans: the oracle's status decides what the kernels have to report")
    lw = body(400, "dir")
    ql = int(qpre(lw)[-1])
    for d in (-1, 0, 1):
        rw = body(31, f"dirr{d}")
        qr = int(qpre(rw)[-1])
        if (ql - qr) % 2:
            rw = rw.copy()
            rw[0] += 16
            qr += 1
        for sl in "+-":
            for sr in "+-":
                c.add_pair(lw, rw, sl, sr, b0=(ql - qr) // 2 + d, note=f"xa - (Qtot - 1 - xb) = {2 * d}")
    lw = body(215, "c0fit", {0: (EQ, 400), 3: (EQ, 2)})
    rw = body(150, "c0fitr")
    for sr in "+-":
        c.add_pair(lw, rw, "+", sr, b0=int(qpre(lw)[3]), note="backwards into step 0, region [0, ib + 17)")
    return c


def case_checkpoints():
    """item 7: regions of 1025, 4097 and 6000 ops (the 64-ary descent of rb_tw_find: 65, 257, 375 chunks -- strides 2, 5, 6 with a last
    group of 1, 2, 3 chunks, which holds the record's last op); the overlap's ends in the first and the last chunk, and on the first op of a
    chunk (its query prefix is the checkpoint's value)"""
    c = Case("checkpoints", 7)
    for n in (1025, 4097, 6000):
        c.plant(body(n, "cp", {5: (EQ, 2)}, maxlen=2), "tail", 5, j=1, note=f"region {n}: first chunk .. last chunk")
        c.plant(body(n, "cp", {n - 6: (EQ, 2)}, maxlen=2), "head", n - 6, note=f"region {n}: op 0 .. last chunk")
    c.plant(body(1057, "cpq", {48: (EQ, 2)}, maxlen=2), "tail", 48, j=0, note="staged whole under 6144: xa == checkpoint 3")
    c.plant(body(6400, "cpq", {2320: (EQ, 2)}, maxlen=2), "tail", 2320, j=0, note="region [2304, 6400), 256 chunks: xa == checkpoint 1")
    return c


# ---- pairs from per-base strings (items 8 and 9) ---------------------------------------------------------------------------------------
CH = {"=": EQ, "X": X, "M": M, "I": I, "d": D, "n": N}


def _rle(tokens):
    out = []
    for t in tokens:
        if out and out[-1][0] == CH[t]:
            out[-1][1] += 1
        else:
            out.append([CH[t], 1])
    return record([(c, ln) for c, ln in out])


def string_pair(c, l_head, l_ov, r_ov, r_tail, note=""):
    """four pairs (the strand combinations) from per-base strings in QUERY order: the left record is l_head + l_ov, the right one r_ov + r_tail,
    the overlap the o = len(l_ov) = len(r_ov) bases between.  = X M I are query bases; d / n are units of a D / N op that lies between two
    bases (an overlap string may hold them: they are not counted).  On '-' the ops are the run lengths of the reversed string."""
    nq = lambda s: sum(ch in "=XMI" for ch in s)  # noqa: E731
    assert nq(l_ov) == nq(r_ov)
    for sl in "+-":
        for sr in "+-":
            lt, rt = l_head + l_ov, r_ov + r_tail
            c.add_pair(_rle(lt if sl == "+" else lt[::-1]), _rle(rt if sr == "+" else rt[::-1]), sl, sr, o=nq(l_ov), note=note)


def alt(k, a="X", b="M"):
    return "".join((a, b)[i & 1] for i in range(k))


def base_scores(s, scores):
    """the score of every query base of a string without D / N (score_of_qpos: = scores match, I -indel, X and M -diff)"""
    ms, ds, is_ = scores
    return np.array([ms if ch == "=" else (-is_ if ch == "I" else -ds) for ch in s], np.int64)


def f_values(l_ov, r_ov, scores):
    """f(k) = l[0 .. k) + r[k .. n), k = 0 .. n (trim_overlap.rs:50-76), for overlap strings without D / N"""
    l, r = base_scores(l_ov, scores), base_scores(r_ov, scores)
    return np.concatenate([[0], np.cumsum(l)]) + np.concatenate([np.cumsum(r[::-1])[::-1], [0]])


def first_strict_max(f):
    """(index, value): the split's rule -- the first strict maximum, starting from 0 at index 0"""
    best, idx = 0, 0
    for k, v in enumerate(f):
        if v > best:
            best, idx = int(v), k
    return idx, best


def case_ties():
    """item 8: split ties and degenerate maxima, scores (1, 1, 1).  `small`: records of 20 .. 60 ops (the row form: candidates in different
    lane chunks); `large`: the overlap spans more than 128 ops of both records (the wave form: candidates 64 ops apart -- one lane -- and
    70 apart -- two lanes).  Each entry: (l_ov, r_ov, property)."""
    c = Case("ties", 8, scores=((1, 1, 1),))
    c.strings = []

    def add(l_ov, r_ov, prop, head="==X=M=X==", tail="==X=M=X=="):
        c.strings.append((l_ov, r_ov, prop, len(c.left)))
        string_pair(c, head, l_ov, r_ov, tail, note=prop)

    add(alt(14) + "=" + alt(15), alt(10) + "=" + alt(19, "M", "X"), "all f <= 0 and f(0) < 0")
    add(alt(30), alt(30, "M", "X"), "flat")
    add("=" * 30, "=" * 30, "flat and positive")
    add("=" * 5 + alt(20, "=", "I") + "=====", alt(30), "maximum only at k = n")
    # rise to the maximum at a, fall, rise to the same maximum at a + 2 b, fall: the smaller k wins
    twice = lambda a, b, z: ("=" * a + alt(b) + "=" * b + alt(z), alt(a) + "=" * b + alt(b) + "=" * z)  # noqa: E731
    add(*twice(6, 12, 8), "the maximum twice (small)")
    add(*twice(10, 63, 80), "the maximum twice, 64 ops apart (large)", head="==" + alt(60, "X", "="), tail=alt(60, "=", "X") + "==")
    add(*twice(10, 70, 80), "the maximum twice, 70 ops apart (large)", head="==" + alt(60, "X", "="), tail=alt(60, "=", "X") + "==")
    # the right record's score changes under a run of the left record: f rises to the maximum and stays there (boundaries of one record only)
    add("=" * 30, alt(11) + "=" * 19, "a plateau behind the maximum")
    add("=" * 12 + alt(18), alt(12) + "=" * 18, "the maximum where both records' op boundaries coincide")
    return c


def case_special_max():
    """item 8, the maximum on a special last base: a D run behind a query op gives the op's last base (in op order) the run's score, so the left
    record's f rises up to that base only; both policies"""
    c = Case("special_max", 8, scores=((1, 1, 1), (2, 3, 5)))
    string_pair(c, "==X==", "=" * 9 + "dd" + alt(11), alt(10) + "=" * 10, "==X==", note="D behind the left record's rising run")
    string_pair(c, "==X==", "=" * 10 + alt(10), alt(6) + "ddd" + alt(4) + "=" * 10, "==X==", note="D inside the right record's falling run")
    return c


def case_one_op():
    """item 9: the split inside a record's first or last op, a clip that keeps one op, a record of one op"""
    c = Case("one_op", 9, in_place=True)
    string_pair(c, "==", "=" + alt(11), "=" * 12, "==X=M==", note="split at 0: the left clip is two bases of one op")
    string_pair(c, "==X=M==", "=" * 12, alt(12), "==", note="split at n: the right clip is two bases of one op")
    string_pair(c, "==X==", "=" * 11 + "X", alt(11) + "=", "===X==", note="split at n - 1: inside the last overlapped ops")
    string_pair(c, "==X==", "=" + alt(11), "X" + "=" * 11, "===X==", note="split at 1")
    string_pair(c, "=" * 6, "=" * 4, alt(4), "=X==", note="a left record of one op, kept whole")
    string_pair(c, "==X=", alt(4), "=" * 4, "=" * 6, note="a right record of one op, kept whole")
    string_pair(c, "=" * 6, "=" * 4, "====", "=" * 5, note="two records of one op")
    return c


def case_statuses():
    """item 12: spans that touch, lie apart, or contain one another, on records of 193 and 1025 ops.  rb_pair_open lists the touching and the
    apart pair (decline 2: no overlap); a right record inside the left one goes as far as the clips, and where it starts with the left one the
    left clip is empty (`bad`, decline 5).  The oracle's status (STATUS_OF: the reference cuts the touching and the inner pair, and panics on
    the other two) has to come out whichever attempt ends up with the pair"""
    c = Case("statuses", 12, route_open="statuses other than OK are the subject", status=None)
    for n in (193, 1025):
        lw, rw, inner = body(n, "stl"), body(n, "str"), body(61, "sti")
        ql = int(qpre(lw)[-1])
        for sl in "+-":
            for sr in "+-":
                c.add_pair(lw, rw, sl, sr, b0=ql, note=f"touching n={n}")
                c.add_pair(lw, rw, sl, sr, b0=ql + 17, note=f"apart n={n}")
                c.add_pair(lw, inner, sl, sr, b0=(ql - int(qpre(inner)[-1])) // 2, note=f"contained n={n}")
                c.add_pair(lw, inner, sl, sr, b0=0, note=f"contained_start n={n}")
    return c


STATUS_OF = {"touching": 0, "contained": 0, "contained_start": 16, "apart": 21}  # 16: RB_ST_PANIC_NOTFOUND, 21: RB_ST_PANIC_ASSERT


def walker_batch(n_short=12288, n_slab=64):
    """item 11: n_short pairs the 64-op row form declines and the 128-op one takes (140-op records, the overlap spans 70 .. 100 ops) and, one
    every n_short / n_slab pairs, a pair whose overlap spans 6200 .. 7000 ops of a 7100-op record: more than the 6144 ops of the last LDS
    attempt, so only the slab attempt (48 workgroups, 64 list entries each per round) can hold it.  Templates are built once and laid out
    again and again: every pair still has records of its own in the batch.  -> (args, left, right, is_slab, the two template cases)"""
    rng = np.random.default_rng(11)
    short, slab = Case("walker_short", 11), Case("walker_slab", 11)
    for k in range(8):
        span, end = int(rng.integers(70, 101)), ("tail", "head")[k & 1]
        far = 140 - span if end == "tail" else span - 1
        short.plant(body(140, f"ws{k}", {far: (EQ, 2)}), end, far, seed=k)
    for k in range(4):
        span, end = (6200, 6999, 6500, 6800)[k], ("tail", "head")[k & 1]
        far = 7100 - span if end == "tail" else span - 1
        slab.plant(body(7100, f"wl{k}", {far: (EQ, 2)}, maxlen=2), end, far, seed=k)
    every = n_short // n_slab
    cols = {k: [] for k in ("t_st", "t_en", "q_st", "q_en", "strand")}
    cigs, left, right, is_slab = [], [], [], []

    def put(case, i):
        b, l, r = case.batch()
        for rec in (int(l[i]), int(r[i])):
            cigs.append(case.cigs[rec])
            for k in cols:
                cols[k].append(b[k][rec])
        left.append(len(cigs) - 2); right.append(len(cigs) - 1)

    ns, nl = len(short.left), len(slab.left)
    for i in range(n_short):
        if i % every == every // 2 and len(is_slab) - i < n_slab:
            put(slab, (i // every) % nl)
            is_slab.append(True)
        put(short, i % ns)
        is_slab.append(False)
    off = np.zeros(len(cigs) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in cigs])
    args = (np.concatenate(cigs), off, *[np.array(cols[k], np.uint64) for k in ("t_st", "t_en", "q_st", "q_en")], np.array(cols["strand"], np.uint8))
    return args, np.array(left, np.uint32), np.array(right, np.uint32), np.array(is_slab), short, slab


CASES = {
    "row_length": case_row_length, "row_edge": case_row_edge, "row_chunks": case_row_chunks, "wave_length": case_wave_length,
    "wave_fit_192": lambda: case_wave_fit(192), "wave_fit_1024": lambda: case_wave_fit(1024), "wave_fit_6144": lambda: case_wave_fit(6144),
    "wave_fit_32768": lambda: case_wave_fit(32768), "wave_steps": case_wave_steps, "wave_direction": case_wave_direction,
    "checkpoints": case_checkpoints, "ties": case_ties, "special_max": case_special_max, "one_op": case_one_op, "statuses": case_statuses,
}
_made = {}


def case(name):
    """the case, built once per process"""
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]
