"""Helpers of the generic wave clip kernel's tests (tests/test_generic_inputs.py, tests/test_gpu_generic_wave.py).

Two things, neither taken from the kernels' output:
  * builders: records and window lists placed on the geometry of rb_k_generic_checkpoints / rb_k_generic_jobs /
              rb_k_liftover_generic_wave (k_liftover.hip): a checkpoint in front of every 64th kept op (RB_GCP), steps of 64 ops, 256 ops
              per load group of the checkpoint kernel, 64 checkpoints per ballot of cp_search;
  * Model:    the kernel's DECISIONS restated in plain Python / numpy over per-op and per-unit arrays -- which checkpoints a hit starts
              and resumes at (k1, k2, k3), whether the jumps of pass 1 and pass 2 are taken, whether pass 2 needs its second attempt,
              whether an equal range straddles a checkpoint, which steps of pass 3 are fast or general and whether a run is carried from
              step to step -- together with the row and the clip those decisions lead to (modern policy), so that the CPU test can hold
              the model itself against the per-base oracle.
A "unit" is one element of the reference's tpos_aln / qpos_aln: an op of length L holds L of them (paf.rs:505-534)."""
import numpy as np

from rbtest_util import CONT, OPC, QRY, REF

GCP, STEP, WALK_MAX = 64, 64, 24            # RB_GCP, ops per step of the wave kernel, RB_WALK_MAX (rb_lift.h)
M, I, D, N, S, H, P, EQ, X = (OPC[c] for c in "MIDNSHP=X")
MATCH = (M, EQ, X)
ST_OK, ST_NONE_INDEL, ST_NOTFOUND = 0, 1, 16
HIT_INSIDE, HIT_GENERIC, HIT_DESCRIPTOR = 1, 2, 4


def op(ln, code):
    return (ln << 4) | code


# ------------------------------------------------------------------------------------------------ CIGAR makers
_MID = ((1, X), (2, I), (3, D), (5, N))


def alt(count, match_first, k0=0, max_len=9):
    """`count` regular ops, match ops (=) and X / I / D / N in turn, beginning with a match op or not; no two neighbours of one type"""
    out = []
    for k in range(count):
        j = (k0 + k) // 2
        if (k % 2 == 0) == bool(match_first):
            out.append(op(1 + (3 + j) % max_len, EQ))
        else:
            ln, c = _MID[j % 4]
            out.append(op(min(ln, max_len), c))
    return out


def regular(n, max_len=9):
    """a regular CIGAR of n ops with a match op at both ends"""
    ops = alt(n, True, max_len=max_len)
    if n % 2 == 0:                              # (its last op is X / I / D / N: an X behind the = in front of it)
        ops[-1] = op(2, X)
    return ops


def irregular(n, max_len=9):
    """regular(n - 1) with one more = op put behind the = at index 10: ONE pair of adjacent ops of one type (indices 10 and 11)"""
    ops = regular(n - 1, max_len)
    assert (ops[10] & 15) == EQ and (ops[11] & 15) != EQ
    return ops[:11] + [op(2, EQ)] + ops[11:]


# the structured record: what sits where (indices among the kept ops)
EQ_RUN = (60, 67)            # eight adjacent = ops: a merge across checkpoint 64
DI_RUN = (100, 249)          # 150 ops, D and I in turn: no match op
AT_256 = 256                 # an I op at a checkpoint, a match op in front of it
ZEROS = (260, 265)           # 5= 0= 6= 0I 2I 7=
ZERO_AT = 320                # a zero-length op at a checkpoint
X_RUN = (321, 450)           # 130 adjacent X ops of one base: the step 384 .. 447 lies inside one run
N_STRUCT = 455


def structured(irregular_form=True):
    """the record of 455 ops; irregular_form=False: the regular copy (the D / I run, no equal neighbours, no zero length)"""
    o = alt(60, True)                                                                  # 0 .. 59, a match op first, X / I / D / N at 59
    o += [op(ln, EQ if irregular_form or k % 2 else X) for k, ln in enumerate((2, 3, 1, 4, 2, 1, 3, 2))]  # 60 .. 67
    o += alt(32, False, k0=1)                                                          # 68 .. 99, a match op at 99
    o += [op(1 + k % 3, D if k % 2 == 0 else I) for k in range(150)]                   # 100 .. 249
    o += [op(4, EQ), op(1, X), op(2, D), op(3, EQ), op(2, I), op(5, EQ), op(3, I), op(4, EQ), op(2, D), op(2, X)]  # 250 .. 259
    if irregular_form:
        o += [op(5, EQ), op(0, EQ), op(6, EQ), op(0, I), op(2, I), op(7, EQ)]          # 260 .. 265
    else:
        o += [op(5, EQ), op(1, X), op(6, EQ), op(1, D), op(2, I), op(7, EQ)]
    o += alt(54, False, k0=1)                                                          # 266 .. 319, a match op at 319
    o += [op(0 if irregular_form else 1, I)]                                           # 320
    o += [op(1, X if irregular_form or k % 2 == 0 else EQ) for k in range(130)]        # 321 .. 450
    o += [op(2, D), op(4, EQ), op(1, I), op(6, EQ)]                                    # 451 .. 454
    assert len(o) == N_STRUCT
    return o


STRUCT_MARKS = [59, 60, 61, 63, 64, 65, 67, 68, 99, 100, 101, 249, 250, 251, 255, 256, 257, 259, 260, 261, 262, 263, 264, 265, 266,
                319, 320, 321, 322, 383, 384, 385, 447, 448, 449, 450, 451, 452]
LENGTHS = (63, 64, 65, 128, 129, 256, 257)
N_LONG = 4300
LEAD = [op(2, I), op(3, I), op(1, I)]       # stripped by remove_trailing_indels: first_op = 3 (insertions only: a leading D moves the
                                            # reference's coordinates by more than its bases, paf.rs:668-701, and the record's would not add up)


def records(t0):
    """-> list of (name, ops).  t0 == 0 adds the records whose first unit consumes no reference (their tpos_aln is not sorted)."""
    recs = [(f"len{n}", irregular(n)) for n in LENGTHS]
    recs += [("struct", structured(True)), ("struct_regular", structured(False)), ("stripped", LEAD + irregular(130)),
             ("long", irregular(N_LONG, max_len=3))]
    if t0 == 0:
        recs += [("lead_3S", [op(3, S)] + irregular(199)), ("lead_2H", [op(2, H)] + regular(199)),
                 ("lead_zeros_4S", [op(0, (EQ, X, N)[k % 3]) for k in range(70)] + [op(4, S)] + regular(127)),
                 # units at position -1 over a third of the record: the probe sequence of the binary search runs into them
                 ("lead_400S", [op(400, S)] + irregular(199))]
    return recs


def batch(t0, strand):
    """one contig, every record at t_st = t0"""
    recs = records(t0)
    n = len(recs)
    cigs = [np.array(c, np.uint32) for _, c in recs]
    op_off = np.zeros(n + 1, np.uint64)
    op_off[1:] = np.cumsum([len(c) for c in cigs])
    R = np.array([int(sum(int(v) >> 4 for v in c if (int(v) & 15) in REF)) for c in cigs], np.uint64)
    Q = np.array([int(sum(int(v) >> 4 for v in c if (int(v) & 15) in QRY)) for c in cigs], np.uint64)
    t_st = np.full(n, t0, np.uint64)
    q_st = np.arange(n, dtype=np.uint64) * 7
    return dict(ops=np.concatenate(cigs), op_off=op_off, t_st=t_st, t_en=t_st + R, q_st=q_st, q_en=q_st + Q,
                strand=np.full(n, ord(strand), np.uint8), contig=np.zeros(n, np.uint32), names=[nm for nm, _ in recs])


# ------------------------------------------------------------------------------------------------ the model
class Rec:
    """one NORMALISED record (first_op / n_ops / t_st / t_en of the oracle's norm row) as per-op and per-unit arrays"""

    def __init__(self, b, r, norm_row):
        o0 = int(b["op_off"][r]) + int(norm_row["first_op"])
        self.r, self.name = r, b["names"][r]
        self.ops_off, self.n = o0, int(norm_row["n_ops"])
        self.words = b["ops"][o0:o0 + self.n].astype(np.int64)
        self.code, self.len = self.words & 15, self.words >> 4
        assert not (self.code == CONT).any()
        self.t_st, self.t_en, self.q_st, self.q_en = (int(norm_row[k]) for k in ("t_st", "t_en", "q_st", "q_en"))
        self.minus = int(b["strand"][r]) == ord("-")
        self.isref, self.isq, self.ism = (np.isin(self.code, tuple(s)) for s in (REF, QRY, MATCH))
        pre = lambda v: np.concatenate([[0], np.cumsum(v)])  # noqa: E731 (exclusive prefixes, one entry more than ops)
        self.U, self.R, self.Q, self.Mp = pre(self.len), pre(self.len * self.isref), pre(self.len * self.isq), pre(self.len * self.ism)
        self.N = int(self.U[-1])
        # tpos_aln: a reference op's units hold the positions behind the one in front of it, any other op's units repeat that one
        op_of = np.repeat(np.arange(self.n), self.len)
        within = np.arange(self.N) - self.U[op_of]
        self.op_of = op_of
        self.tpos = self.t_st - 1 + self.R[op_of] + np.where(self.isref[op_of], within + 1, 0)
        self.ncp = -(-self.n // GCP)
        self.has_cp = self.n > GCP
        kept = np.flatnonzero(self.len != 0)
        self.wrapped = self.t_st == 0 and len(kept) > 0 and not self.isref[kept[0]]       # units at position -1 come first
        self.irregular = bool((~np.isin(self.code, (M, I, D, N, EQ, X))).any() or (self.len == 0).any() or (self.code[1:] == self.code[:-1]).any()
                              or self.code[0] not in MATCH or self.code[-1] not in MATCH)

    def P(self, k):
        """position of the first reference base at or behind kept op k"""
        return self.t_st + int(self.R[k])

    def last_le(self, target):
        """rb_k_generic_jobs: the last checkpoint with at most `target` reference bases in front of it, by bisection"""
        lo, hi = 0, self.ncp
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if int(self.R[mid * GCP]) <= target:
                lo = mid
            else:
                hi = mid
        return lo

    def cp_search_units(self, target):
        """rb_k_liftover_generic_wave: the last checkpoint with at most `target` units in front of it"""
        ucp = self.U[0:self.n:GCP][:self.ncp]
        return int(np.searchsorted(ucp, target, side="right")) - 1

    def decide(self, wst, wen):
        """what the kernels decide for the window [wst, wen) (which overlaps the record), modern policy"""
        d = dict(inside=False, status=ST_OK, k1=0, k2=0, k2_job=0, k3=0, jump1=False, jump2=False, second=False, straddle=False,
                 steps=[], carried=False, no_start=False, wrapped=self.wrapped, clip=None)
        if self.t_st > wst and self.t_en < wen:
            d["inside"] = True
            d["clip"] = self.words.copy()
            return d
        ps, pe = max(wst, self.t_st), min(wen, self.t_en) - 1
        d["ps"], d["pe"] = ps, pe
        if self.has_cp:
            d["k1"] = self.last_le(ps - self.t_st)
            d["k2"] = self.last_le(pe - self.t_st) if pe >= ps else 0
            d["k2_job"] = d["k2"] if d["k2"] > d["k1"] + 1 else 0
        if self.wrapped:
            return d                                               # (the serial replay's business)
        c_start, c_end1 = d["k1"] * GCP, d["k2_job"] * GCP
        # ---- pass 1: the steps walked, and the jump
        c0 = c_start
        while c0 < self.n:
            Rb = int(self.R[min(c0 + STEP, self.n)])
            if self.t_st - 1 + Rb > pe:
                break
            if c_end1 > c0 + STEP and self.t_st - 1 + Rb > ps:
                d["jump1"] = True
                c0, c_end1 = c_end1 - STEP, 0
            c0 += STEP
        s, e = np.flatnonzero(self.tpos == ps), np.flatnonzero(self.tpos == pe)
        if len(s) == 0 or len(e) == 0:
            d["status"] = ST_NOTFOUND
            return d
        s_lo, s_hi, e_lo, e_hi = int(s[0]), int(s[-1]), int(e[0]), int(e[-1])
        d["equal"] = (s_lo, s_hi, e_lo, e_hi)
        if self.has_cp:                                            # an equal range with ops on both sides of a checkpoint
            for lo, hi in ((s_lo, s_hi), (e_lo, e_hi)):
                a, b = int(self.op_of[lo]), int(self.op_of[hi])
                d["straddle"] |= a // GCP != b // GCP
        ks, ke = s_hi, e_hi
        d["ks"], d["ke"] = ks, ke
        # ---- pass 2
        c_end2 = 0
        if self.has_cp and ke >= ks:
            d["k3"] = self.cp_search_units(ke)
            if d["k3"] * GCP > c_start + GCP:
                c_end2 = d["k3"] * GCP
        for attempt in (0, 1):
            if attempt:
                c_end2, d["second"] = 0, True
            a_set = b_set = jumped = False
            a, b, ia, ib = self.N, 0, 0, 0
            c0 = c_start
            while c0 < self.n:
                if a_set and int(self.U[c0]) > ke:
                    break
                i = np.arange(c0, min(c0 + STEP, self.n))
                live = self.ism[i] & (self.len[i] != 0)
                if not a_set:
                    m = i[live & (self.U[i] + self.len[i] > ks)]
                    if len(m):
                        ia, a_set = int(m[0]), True
                        a = max(ks, int(self.U[ia]))
                m = i[live & (self.U[i] <= ke)]
                if len(m):
                    ib, b_set = int(m[-1]), True
                    b = min(int(self.U[ib]) + int(self.len[ib]) - 1, ke)
                if a_set and c_end2 > c0 + STEP:
                    c0, c_end2, jumped, b_set = c_end2 - STEP, 0, True, False
                    d["jump2"] = True
                c0 += STEP
            if not jumped or b_set:
                break
        if a > b or a >= self.N or not a_set or not b_set:
            d["status"] = ST_NONE_INDEL
            return d
        d.update(a=a, b=b, ia=ia, ib=ib)
        Ra, Qa, Ma = (int(p[ia]) + a - int(self.U[ia]) for p in (self.R, self.Q, self.Mp))
        nRb, nQb, nMb = (int(p[ib]) + b - int(self.U[ib]) + 1 for p in (self.R, self.Q, self.Mp))
        d["row"] = dict(t_st=self.t_st + Ra, t_en=self.t_st + nRb, nmatch=nMb - Ma, aln_len=b - a + 1,
                        q_st=self.q_en - nQb if self.minus else self.q_st + Qa, q_en=self.q_en - Qa if self.minus else self.q_st + nQb)
        # ---- pass 3: ops ia .. ib in steps of 64 from the step that holds ia; a run is carried from step to step
        out, carry = [], None                                     # carry: [bases, code] of the run still open
        for c0 in range(ia & ~63, ib + 1, STEP):
            i = np.arange(c0, c0 + STEP)
            inr = (i >= ia) & (i <= ib)
            j = np.where(inr, i, 0)
            code, ln = np.where(inr, self.code[j], 0), np.where(inr, self.len[j], 0)   # (what lies outside the range loads as a zero word)
            piece = ln.copy()
            if ia == ib:
                piece[i == ia] = b - a + 1
            else:
                piece[i == ia] = int(self.U[ia]) + int(self.len[ia]) - a
                piece[i == ib] = b - int(self.U[ib]) + 1
            ptype = np.concatenate([[carry[1] if carry else 0xFF], code[:-1]])
            odd = inr & ((ln == 0) | ((ptype == code) & ((np.arange(STEP) == 0) | (i > ia))))
            kept = inr & (ln != 0)
            first = np.flatnonzero(kept)
            if carry and len(first) and carry[1] == int(code[first[0]]):
                d["carried"] = True
            if not odd.any():
                d["steps"].append("fast")
                if carry:
                    out.append(carry)
                k = np.flatnonzero(inr)
                out += [[int(piece[x]), int(code[x])] for x in k[:-1]]
                carry = [int(piece[k[-1]]), int(code[k[-1]])]
                continue
            d["steps"].append("general")
            nstarts = 0
            for x in first:
                if carry and carry[1] == int(code[x]):
                    carry[0] += int(piece[x])
                else:
                    if carry:
                        out.append(carry)
                    carry = [int(piece[x]), int(code[x])]
                    nstarts += 1
            if nstarts == 0:
                d["no_start"] = True
        out.append(carry)
        d["clip"] = np.array([op(ln, c) for ln, c in out], np.int64)
        return d


def model_records(oracle, b):
    from rbtest_util import batch_args
    norm = oracle.normalize(oracle.Batch(*batch_args(b), b["contig"]))
    return norm, [Rec(b, r, norm[r]) for r in range(len(norm))]


# ------------------------------------------------------------------------------------------------ windows
def marks_of(rec):
    n = rec.n
    if rec.name == "long":                                           # (every 64th op of 4300 would be 200 marks)
        ks = [0, 1, 64, 128, 192, 256, 512, 1024, 2048, 4096] + [GCP * k for k in (63, 64, 65, 66)]
    else:
        ks = [0, 1] + list(range(GCP, n + 1, GCP)) + list(range(256, n + 1, 256))
    m = {0, 1, n - 2, n - 1}
    for k in ks[2:]:
        m |= {k - 1, k, k + 1}
    if rec.name.startswith("struct"):
        m |= set(STRUCT_MARKS)
    return sorted(k for k in m if 0 <= k < n)


def edge_windows(recs, delta):
    """sorted windows that do not overlap, one behind the other: their edges lie `delta` bases off the first reference base of every
    marked op of every record (the records share the contig, so every record meets every window that overlaps it)"""
    pos = sorted({rec.P(k) + delta for rec in recs for k in marks_of(rec)} | {rec.t_en + 5 for rec in recs})
    pos = [x for x in pos if x >= 0]
    st, en = np.array(pos[:-1], np.uint64), np.array(pos[1:], np.uint64)
    return np.zeros(len(st), np.uint32), st, en


def special_windows(recs):
    """the windows that are no edges: long ones over the D / I run and the X run, one-base windows, a window inside one op, the record's
    span and a window strictly around it; sorted by their start (they overlap each other)"""
    w = []
    for rec in recs:
        w += [(rec.t_st, rec.t_en), (rec.t_st - 1, rec.t_en + 1) if rec.t_st else (0, rec.t_en + 1)]
        w += [(rec.P(k), rec.P(k) + 1) for k in (0, rec.n // 2, rec.n - 1)]           # one base
        k = next(k for k in range(rec.n) if rec.len[k] >= 3 and rec.isref[k])
        w.append((rec.P(k) + 1, rec.P(k) + 2))                                         # inside one op
        if rec.name.startswith("struct"):
            lo, hi = DI_RUN
            for a in (2, 30, 70, 99):                                                  # from in front of the D / I run into it
                w += [(rec.P(a), rec.P(k) + 1) for k in (lo + 10, lo + 40, lo + 80, lo + 120, hi - 1)]
            for k in (lo + 2, lo + 30, lo + 60, lo + 100, lo + 140):                   # from inside it to behind it
                w += [(rec.P(k), rec.P(z)) for z in (hi + 3, 300, 400, rec.n - 1)]
            w += [(rec.P(lo + a), rec.P(lo + z)) for a, z in ((2, 148), (10, 100), (40, 60), (70, 140), (1, 70), (66, 130))]  # wholly inside: none
            w += [(rec.P(2), rec.P(k) + 1) for k in (X_RUN[0] + 5, 383, 384, 400, 447, 448, X_RUN[1])]   # from op 2 into the X run
            w += [(rec.P(X_RUN[0] + a), rec.P(X_RUN[0] + z)) for a, z in ((3, 120), (0, 130), (62, 64), (63, 128), (70, 100))]
            w += [(rec.P(ZEROS[0]) + a, rec.P(ZEROS[1]) + z) for a, z in ((0, 1), (2, 0), (5, 3), (6, 7))]
            w += [(rec.P(EQ_RUN[0]) + a, rec.P(EQ_RUN[1]) + z) for a, z in ((0, 2), (1, 1), (3, 0))]
            e = rec.P(AT_256) - 1                                                      # the last reference base in front of the I op at 256:
            w += [(e, e + z) for z in (1, 2, 5, 40)] + [(rec.P(a), e + 1) for a in (2, 200, 250, 254)]   # its equal range straddles the checkpoint
    w = sorted({(a, z) for a, z in w if z > a})
    st, en = np.array([a for a, _ in w], np.uint64), np.array([z for _, z in w], np.uint64)
    return np.zeros(len(st), np.uint32), st, en


def long_windows(rec):
    """the long record: windows whose last base lies just behind checkpoints 63 .. 66, from three different starts"""
    w = [(rec.P(a), rec.P(GCP * k) + z) for k in (63, 64, 65, 66) for z in (1, 2, 3) for a in (2, 700, GCP * 60 + 5)]
    w = sorted(set(w))
    st, en = np.array([a for a, _ in w], np.uint64), np.array([z for _, z in w], np.uint64)
    return np.zeros(len(st), np.uint32), st, en


def unsorted_windows(recs, n_min=200, seed=7):
    """edge and special windows shuffled and repeated to at least n_min: not sorted, more than 64 on the one contig"""
    a, b = edge_windows(recs, 0), special_windows(recs)
    st, en = np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]])
    rep = -(-n_min // len(st))
    st, en = np.tile(st, rep), np.tile(en, rep)
    o = np.random.default_rng(seed).permutation(len(st))
    return np.zeros(len(st), np.uint32), st[o], en[o]


def subset(b, idx):
    """the records idx of a batch, one behind the other"""
    from scan_util import subset as sub
    out = sub(b, idx)
    out["names"] = [b["names"][i] for i in idx]
    return out


def decisions(recs, w):
    """every (record, window) pair that overlaps (paf_overlaps_rgn on the normalised record) -> the model's decision"""
    out = {}
    for rec in recs:
        for k, (st, en) in enumerate(zip(w[1].tolist(), w[2].tolist())):
            if rec.t_en > st and rec.t_st < en:
                out[(rec.r, k)] = rec.decide(st, en)
    return out


def deep_windows(g, w):
    """windows of list w with a boundary whose walk to the next match op of the regular copy g is longer than RB_WALK_MAX ops, with room
    to spare (an op of the D / I run more than 30 ops from both of its ends)"""
    lo, hi = DI_RUN
    out = []
    for k, (st, en) in enumerate(zip(w[1].tolist(), w[2].tolist())):
        if not (g.t_en > st and g.t_st < en) or (g.t_st > st and g.t_en < en):
            continue
        ps, pe = max(st, g.t_st), min(en, g.t_en) - 1
        a = int(np.searchsorted(g.R[1:] + g.t_st, ps, side="right"))        # the reference op that holds ps / pe
        z = int(np.searchsorted(g.R[1:] + g.t_st, pe, side="right"))
        if lo + 30 <= a <= hi - 30 or lo + 30 <= z <= hi - 30:
            out.append(k)
    return out
