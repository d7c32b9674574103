"""Helpers of the record-scan tests (tests/test_scan_inputs.py, tests/test_gpu_scan_rows.py, tests/soak/soak_scan.py).

Three things, none of them taken from the kernels:
  * route():      the routing rule of rb_dev_scan_records restated (include/rustybam_amd.h, rb_ctx_scan_route) -- which batches take the
                  row form and which of their records it lists;
  * flags_ref():  rb_reduce_row.flags / rb_norm_row.flags in plain numpy, from include/rustybam_amd.h and the reference's paf.rs /
                  bamstats.rs (the per-base oracle has no such field);
  * batches():    inputs placed on the geometry of the row form (a record = a row of 16 lanes, a lane = one aligned 16-byte group of 4
                  words per step, a step = 64 words, four steps in flight) -- every boundary length at every start phase, one-defect
                  records, clean records between hostile neighbours, wavefronts of mixed fate, the routing boundary, magnitudes.

What the generator does NOT build, because the packed-word form gives it no single meaning: a record that holds a misplaced
continuation word (a record's first word, or one behind another continuation word) TOGETHER with a well-placed one, and continuation
words whose value is 0 or above 15.
"""
import numpy as np

from rbtest_util import CONT

F_REGULAR, F_STRIPPED, F_HAS_M = 1, 2, 4
M, I, D, N, S, H, P, EQ, X = range(9)
MATCH_CODES, INDEL_CODES, REGULAR_CODES = (M, EQ, X), (I, D), (M, I, D, N, EQ, X)
REF_CODES, QRY_CODES = (M, D, N, EQ, X), (M, I, S, EQ, X)
UNKNOWN_CODES = (9, 10, 11, 12, 13, 15)
U32_MAX = 0xFFFFFFFF

# rb_ctx_scan_route in include/rustybam_amd.h: the row form takes a batch of >= 64 records whose mean is <= 1536 ops (integer division)
# and lists its records of fewer than 4 or more than 2048 ops
ROWS_MIN_REC, ROWS_MEAN_MAX, ROW_MIN_OPS, ROW_MAX_OPS = 64, 1536, 4, 2048
STEP, GROUP, IN_FLIGHT = 64, 4, 4          # words a row takes per step, words per lane and step, steps whose loads are in flight together


def route(op_off):
    """-> (records the row form scans itself, records it lists); (0, 0): the wave-per-record kernel takes the whole batch"""
    n = np.diff(np.asarray(op_off).astype(np.int64))
    if len(n) >= ROWS_MIN_REC and int(op_off[-1]) // len(n) <= ROWS_MEAN_MAX:
        listed = int(((n < ROW_MIN_OPS) | (n > ROW_MAX_OPS)).sum())
        return len(n) - listed, listed
    return 0, 0


# ------------------------------------------------------------------------------------------------ the words of one record
def split_words(words):
    """-> (code, length) per word, int64, with every well-placed continuation word folded into the op in front of it (that op's length
    grows by value << 28, the continuation word keeps code 14 and length 0) and a flag per word: is a folded continuation word.
    Well placed: behind a word of a known code (0..8), value 1..15.  Any other word of a code above 8 stays an op of an unknown code with
    the length it carries (it consumes nothing; its length counts in the unit total alone)."""
    w = np.asarray(words).astype(np.int64)
    code, ln = w & 15, w >> 4
    folded = np.zeros(len(w), bool)
    if len(w) > 1:
        folded[1:] = (code[1:] == CONT) & (code[:-1] <= 8) & (ln[1:] >= 1) & (ln[1:] <= 15)
    k = np.flatnonzero(folded)
    ln = ln.copy()
    ln[k - 1] += ln[k] << 28
    ln[k] = 0
    return code, ln, folded


def sums(words):
    """-> dict(R, Q, M, U, m_len): reference / query / match bases, the unit total (all lengths) and the bases of M ops"""
    code, ln, _ = split_words(words)
    tot = lambda codes: int(ln[np.isin(code, codes)].sum())  # noqa: E731
    return dict(R=tot(REF_CODES), Q=tot(QRY_CODES), M=tot(MATCH_CODES), U=int(ln.sum()), m_len=tot((M,)))


def end_runs(words):
    """-> (lead, trail): the WORDS of the runs of I / D ops at the two ends (remove_trailing_indels, paf.rs:668-723; an op and its
    continuation word are one op of two words)"""
    code, _, folded = split_words(words)
    n = len(code)
    indel = np.isin(code, INDEL_CODES)
    part = indel.copy()                         # the word belongs to an I / D op
    part[1:] |= folded[1:] & indel[:-1]
    lead = n if part.all() else int(np.argmin(part))
    trail = n if part.all() else int(np.argmin(part[::-1]))
    return lead, trail


def flags_of(words):
    """(reduce flags, norm flags of a record whose norm row has status OK) of one record"""
    w = np.asarray(words).astype(np.int64)
    code, raw_len = w & 15, w >> 4
    n = len(w)
    s = sums(words)
    # RB_F_REGULAR: every op code in M I D N = X (so none above 8: a continuation word makes a record irregular), every length >= 1,
    # no two adjacent ops of one code, and the unit total fits the reference's u32 sum (paf.rs:632-647)
    regular = bool(np.isin(code, REGULAR_CODES).all()) and (n == 0 or int(raw_len.min()) >= 1) and \
        not bool((code[1:] == code[:-1]).any()) and s["U"] <= U32_MAX
    has_m = s["m_len"] > 0                      # bamstats.rs:145: `stats.matches > 0`
    red = (F_REGULAR if regular else 0) | (F_HAS_M if has_m else 0)
    norm = red
    if n:
        lead, trail = end_runs(words)
        if lead or trail:
            norm |= F_STRIPPED
        if lead + trail <= n:                   # (otherwise paf.rs:757 panics: no kept range)
            # the kept range must begin and end on M / = / X
            if int(code[lead]) not in MATCH_CODES or int(code[n - 1 - trail]) not in MATCH_CODES:
                norm &= ~F_REGULAR
    return red, norm


def batch_sums(ops, op_off):
    """the same over a whole batch at once: per record R, Q, M, U, m_len, lead, trail (words), the codes of the first and last kept word
    (-1: none) and the number of words that break a rule of RB_F_REGULAR"""
    off = np.asarray(op_off).astype(np.int64)
    n = np.diff(off)
    w = np.asarray(ops).astype(np.int64)[:off[-1]]
    code, raw = w & 15, w >> 4
    first = np.zeros(len(w), bool)
    first[off[:-1][n > 0]] = True
    prev = np.concatenate([[15], code[:-1]])
    folded = (code == CONT) & ~first & (prev <= 8) & (raw >= 1) & (raw <= 15)
    ln = raw.copy()
    k = np.flatnonzero(folded)
    ln[k - 1] += raw[k] << 28
    ln[k] = 0

    def per(v):
        pre = np.concatenate([[0], np.cumsum(v.astype(np.int64))])
        return pre[off[1:]] - pre[off[:-1]]
    out = dict(R=per(ln * np.isin(code, REF_CODES)), Q=per(ln * np.isin(code, QRY_CODES)), M=per(ln * np.isin(code, MATCH_CODES)), U=per(ln),
               m_len=per(ln * (code == M)),
               n_bad=per(~np.isin(code, REGULAR_CODES) | (raw == 0) | ((code == prev) & ~first)))
    indel = np.isin(code, INDEL_CODES)
    part = indel | (folded & np.concatenate([[False], indel[:-1]]))
    stop = np.flatnonzero(~part)                                   # the words that end a run of I / D ops
    j = np.searchsorted(stop, off[:-1])
    has = (j < len(stop)) & (stop[np.minimum(j, max(len(stop) - 1, 0))] < off[1:]) if len(stop) else np.zeros(len(n), bool)
    lead, trail = n.copy(), n.copy()
    if len(stop):
        jl = np.searchsorted(stop, off[1:]) - 1
        lead[has] = (stop[j[has]] - off[:-1][has])
        trail[has] = (off[1:][has] - 1 - stop[jl[has]])
    out["lead"], out["trail"] = lead, trail
    kept = has                                                     # (a record with a kept range: not all indel, not empty)
    fc, lc = np.full(len(n), -1), np.full(len(n), -1)
    fc[kept] = code[off[:-1][kept] + lead[kept]]
    lc[kept] = code[off[1:][kept] - 1 - trail[kept]]
    out["first_code"], out["last_code"] = fc, lc
    return out


def flags_ref(b):
    """-> (reduce flags [n_rec], norm flags [n_rec]) = flags_of for every record of a batch (the norm flags mean something where the norm
    row's status is OK)"""
    s = batch_sums(b["ops"], b["op_off"])
    n = np.diff(np.asarray(b["op_off"]).astype(np.int64))
    regular = (s["n_bad"] == 0) & (s["U"] <= U32_MAX)
    red = np.where(regular, F_REGULAR, 0) | np.where(s["m_len"] > 0, F_HAS_M, 0)
    ends = np.isin(s["first_code"], MATCH_CODES) & np.isin(s["last_code"], MATCH_CODES)
    norm = np.where(regular & (ends | (s["first_code"] < 0)), F_REGULAR, 0) | np.where(s["m_len"] > 0, F_HAS_M, 0) | \
        np.where((n > 0) & ((s["lead"] > 0) | (s["trail"] > 0)), F_STRIPPED, 0)
    return red.astype(np.uint32), norm.astype(np.uint32)


def defects(words):
    """every reason one record is not regular, as (word index, kind) -- for the CPU test that proves a one-defect record has ONE.
    'same' sits at the second word of an equal pair."""
    w = np.asarray(words).astype(np.int64)
    code, ln = w & 15, w >> 4
    out = []
    for i in range(len(w)):
        c = int(code[i])
        if c == CONT:
            out.append((i, "cont"))
            continue                            # (a continuation word's value is not a length; it equals no neighbour)
        if c > 8:
            out.append((i, "unknown"))
        elif c in (S, H, P):
            out.append((i, "SHP"[c - S]))
        if ln[i] == 0:
            out.append((i, "zero"))
        if i and c == int(code[i - 1]):
            out.append((i, "same"))
    return out


# ------------------------------------------------------------------------------------------------ CIGAR makers
_TABLE = np.array([EQ, X, M, I, D, N])


def regular_words(rng, n, long_len=150):
    """a regular CIGAR of n words: M I D N = X, lengths >= 1, no two neighbours of one code, M / = / X at both ends"""
    if n == 0:
        return np.zeros(0, np.uint32)
    code = _TABLE[np.cumsum(rng.integers(1, 6, n)) % 6]            # steps of 1..5 in a cycle of 6: neighbours differ
    if n == 1:
        code[0] = EQ
    elif n == 2:
        code[:] = (EQ, X)
    else:
        code[0] = next(c for c in (EQ, X, M) if c != code[1])
        code[-1] = next(c for c in (EQ, X, M) if c != code[-2])
    ln = rng.choice(np.array([1, 2, 3, 9, long_len]), n, p=[.45, .2, .15, .15, .05])
    return ((ln << 4) | code).astype(np.uint32)


def wild_words(rng, n):
    """anything of the nine codes, zero lengths and equal neighbours included (a defect at almost every position)"""
    code = rng.choice(9, n, p=[.1, .12, .12, .04, .03, .03, .03, .38, .15])
    ln = rng.choice(np.array([0, 1, 2, 3, 7, 40]), n, p=[.04, .4, .2, .16, .15, .05])
    return ((ln << 4) | code).astype(np.uint32)


def base3_words(n):
    """a regular CIGAR of n >= 4 words in which a word differs from BOTH words in front of it (so setting word i to the code of
    word i - 1 makes one equal pair, not two), M / = / X in the last two places"""
    assert n >= 4
    code = np.array([EQ, X, I, EQ, X, D])[np.arange(n) % 6]
    code[n - 2] = next(c for c in (EQ, X, M) if c not in (code[n - 3], code[n - 4]))
    code[n - 1] = next(c for c in (EQ, X, M) if c not in (code[n - 2], code[n - 3]))
    ln = 1 + (np.arange(n) * 7) % 9
    return ((ln << 4) | code).astype(np.uint32)


DEFECTS = ("same", "zero", "S", "H", "P", "unknown", "cont")


def with_defect(words, i, kind, k=0):
    """base3_words with exactly one defect at word i.  k picks the unknown code / the continuation word's value."""
    w = words.copy()
    code, ln = int(w[i]) & 15, int(w[i]) >> 4
    if kind == "same":
        j = i - 1 if i else 1
        w[i] = (ln << 4) | (int(w[j]) & 15)
    elif kind == "zero":
        w[i] = code
    elif kind in "SHP":
        w[i] = (ln << 4) | (S + "SHP".index(kind))
    elif kind == "unknown":
        w[i] = (ln << 4) | UNKNOWN_CODES[k % len(UNKNOWN_CODES)]
    elif kind == "cont":                       # behind a real op for i >= 1 (that op grows by value << 28), a record's first word for i = 0
        w[i] = ((1, 9, 15, 8)[k % 4] << 4) | CONT
    else:
        raise ValueError(kind)
    return w


def defect_positions(n, head):
    """the word indices of the issue: 0, 3, 4 (a lane's last word and the next lane's first when the record starts on a group boundary),
    63 - head, 64 - head (the last word of a row's first step and the first of its second), 255, 256, n - 2, n - 1"""
    return sorted({i for i in (0, 3, 4, STEP - 1 - head, STEP - head, 255, 256, n - 2, n - 1) if 0 <= i < n})


# ------------------------------------------------------------------------------------------------ batches
class Builder:
    """records one behind the other in ops[]; tags[r] says what record r is there for"""

    def __init__(self, rng):
        self.rng, self.recs, self.tags, self.coord, self.strand, self.n_ops = rng, [], [], [], [], 0

    def phase(self):
        return self.n_ops % GROUP

    def add(self, words, tag=None, strand=None, coord="ok"):
        words = np.asarray(words, np.uint32)
        self.recs.append(words)
        self.tags.append(tag or {})
        self.coord.append(coord)
        self.strand.append(strand if strand is not None else "+-"[len(self.recs) % 2])
        self.n_ops += len(words)
        return len(self.recs) - 1

    def filler(self, n=None):
        return self.add(regular_words(self.rng, n if n is not None else int(self.rng.integers(4, 40))), {"kind": "filler"})

    def to_phase(self, p):
        """a filler record of 4..7 words behind which the next record starts at op_off mod 4 == p"""
        self.filler(4 + (p - self.n_ops) % GROUP)
        assert self.phase() == p

    def pad_records(self, n_rec):
        while len(self.recs) < n_rec:
            self.filler()

    def finish(self):
        n = len(self.recs)
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum([len(c) for c in self.recs])
        t_st = self.rng.integers(0, 3000, n).astype(np.uint64)
        q_st = self.rng.integers(0, 3000, n).astype(np.uint64)
        ops = np.concatenate(self.recs) if n else np.zeros(0, np.uint32)
        s = batch_sums(ops, off)
        t_en, q_en = t_st + s["R"].astype(np.uint64), q_st + s["Q"].astype(np.uint64)
        for r, how in enumerate(self.coord):
            if how == "ok":
                continue
            if how == "t_en+1":
                t_en[r] += 1
            elif how == "q_en+2":
                q_en[r] += 2
            elif how == "t_inverted":                              # t_en < t_st
                t_st[r], t_en[r] = 5000, 4999
            elif how == "q_inverted":
                q_st[r], q_en[r] = 7, 0
            else:
                raise ValueError(how)
        return dict(ops=ops, op_off=off, t_st=t_st, t_en=t_en, q_st=q_st, q_en=q_en,
                    strand=np.array([ord(s) for s in self.strand], np.uint8), contig=np.zeros(n, np.uint32), tags=self.tags)


BOUNDARY_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17] + [c + d for c in (64, 128, 256, 1024, 2048) for d in range(-4, 5)]
LONG_LENGTH = 6001


def lengths_batch(rng, mode):
    """every boundary length at every start phase op_off mod 4, plus one record of ~6000 words"""
    B = Builder(rng)
    make = regular_words if mode == "regular" else wild_words
    for n in BOUNDARY_LENGTHS:
        for p in range(GROUP):
            B.to_phase(p)
            B.add(make(rng, n), {"kind": "length", "n": n, "phase": p})
    B.add(make(rng, LONG_LENGTH), {"kind": "length", "n": LONG_LENGTH, "phase": B.phase()})
    B.filler()
    return B.finish()


def fate_batch(rng):
    """wavefronts (four consecutive records, the first at a multiple of four) of mixed fate; the last wavefront has one live row and
    n_rec is a multiple of neither 4 nor 16"""
    B = Builder(rng)
    B.pad_records(8)
    for quad in ((2048, 4, 3, 2049), (3, 2, 500, 2049), (0, 1, 2, 3), (2049, 2050, 6001, 2048), (4, 2048, 4, 2048)):
        assert len(B.recs) % 4 == 0
        for n in quad:
            B.add(regular_words(rng, n), {"kind": "fate", "quad": quad})
    B.pad_records(77)
    return B.finish()


def routing_batches(rng):
    """the routing boundary: 63 and 64 records of the same shape; 64 records with batch means of exactly 1536, 1536 + 63 / 64 and 1537"""
    out = {}
    for n_rec in (63, 64):
        B = Builder(rng)
        B.pad_records(n_rec)
        out[f"route_{n_rec}_records"] = B.finish()
    for name, total in (("route_mean_1536", 1536 * 64), ("route_mean_1536_63", 1536 * 64 + 63), ("route_mean_1537", 1537 * 64)):
        B = Builder(rng)
        for r in range(63):
            B.add(regular_words(rng, 1530 + r % 13), {"kind": "filler"})
        B.add(regular_words(rng, total - B.n_ops), {"kind": "filler"})
        assert 1500 < len(B.recs[-1]) <= ROW_MAX_OPS
        out[name] = B.finish()
    return out


def defect_batch(rng, n, positions=None):
    """per start phase: a clean record of n words, then the same record with exactly one defect, for every position and kind"""
    B = Builder(rng)
    base = base3_words(n)
    k = 0
    for head in range(GROUP):
        B.to_phase(head)
        B.add(base, {"kind": "clean", "n": n, "head": head})
        for i in (positions(n, head) if positions else defect_positions(n, head)):
            for kind in DEFECTS:
                B.to_phase(head)
                B.add(with_defect(base, i, kind, k), {"kind": "defect", "n": n, "head": head, "at": i, "what": kind})
                k += 1
    B.pad_records(ROWS_MIN_REC)
    return B.finish()


HOSTILE = ("same", "zero", "S", "unknown")


def hostile_batch(rng):
    """a regular record that shares its first and last 16-byte group with its neighbours, whose adjoining words have the same code as
    the record's end words, a zero length, or an irregular code: it stays regular and its sums do not move"""
    B = Builder(rng)
    for n in (4, 5, 61, 130, 2046):
        for head in (1, 2, 3):
            for tail in (1, 2, 3):
                if (head + n) % GROUP != tail:
                    continue
                for kind in HOSTILE:
                    mid = regular_words(rng, n)
                    first, last = int(mid[0]) & 15, int(mid[-1]) & 15
                    bad = {"same": None, "zero": 0, "S": (7 << 4) | S, "unknown": (7 << 4) | 11}[kind]
                    before, after = regular_words(rng, 8), regular_words(rng, 9)
                    before[-1] = (5 << 4) | first if kind == "same" else bad | (first if kind == "zero" else 0)
                    after[0] = (5 << 4) | last if kind == "same" else bad | (last if kind == "zero" else 0)
                    if kind == "same":                              # (the neighbours stay regular themselves)
                        before[-2] = (3 << 4) | next(c for c in (I, D, N) if c != (int(before[-3]) & 15))
                        after[1] = (3 << 4) | next(c for c in (I, D, N) if c != (int(after[2]) & 15))
                    B.to_phase((head - 8) % GROUP)
                    B.add(before, {"kind": "hostile_before", "what": kind})
                    assert B.phase() == head
                    B.add(mid, {"kind": "hostile_mid", "n": n, "head": head, "tail": tail, "what": kind})
                    B.add(after, {"kind": "hostile_after", "what": kind})
    B.pad_records(ROWS_MIN_REC)
    return B.finish()


def _alt(codes, lens):
    lens = np.asarray(lens, np.int64)
    return ((lens << 4) | np.asarray(codes)[np.arange(len(lens)) % len(codes)]).astype(np.uint32)


def _pack(text):
    from rbtest_util import pack
    return pack(text)


def magnitude_batch(rng):
    """sums that cross the 20-bit pieces and the u32 total, continuation words on lane and step boundaries, many events, broken
    coordinates, all-indel records and the end-indel quirks at 4+ words (so that the row form finishes them)"""
    B = Builder(rng)
    big = (1 << 28) - 1
    B.add(_alt((EQ, X), [big] * 2048), {"kind": "overflow_2048"})                       # per-class sums of ~2^38; PANIC_OVERFLOW
    B.add(_alt((EQ, X), [big] * 16 + [15]), {"kind": "total_u32_max"})                   # a unit total of exactly 2^32 - 1
    B.add(_alt((EQ, X), [big] * 16 + [16]), {"kind": "total_2_32"})                      # and of 2^32
    B.add(_alt((I, D), 1 + np.arange(2048) % 5), {"kind": "events_all_indel"})           # 1024 I and 1024 D events; paf.rs:757 panics
    B.add(np.concatenate([_pack("7="), _alt((I, D), 1 + np.arange(2046) % 3), _pack("9=")]), {"kind": "events_1023"})
    for head in range(GROUP):                                                            # continuation words where lanes and steps meet
        w = base3_words(300)
        at = sorted({GROUP - head, 2 * GROUP - head, STEP - head, 2 * STEP - head, IN_FLIGHT * STEP - head, 150})
        for j, i in enumerate(at):
            w[i] = ((9 if i == 150 else 1) << 4) | CONT                                 # (one of 9 << 28: a value with bit 3 set)
        B.to_phase(head)
        B.add(w, {"kind": "cont_boundaries", "head": head, "at": at})
    B.add(_pack("5X3000000000=7X2I4="), {"kind": "cont_3e9"})                            # regular but for its one long op, status OK
    for how in ("t_en+1", "q_en+2", "t_inverted", "q_inverted"):
        B.add(regular_words(rng, 40), {"kind": "broken", "how": how}, coord=how)
    for text in ("2I3D1I4D", "1D2I3D4I5D", "3I1D2I1D3I1D2I1D"):
        for strand in "+-":
            B.add(_pack(text), {"kind": "all_indel"}, strand=strand)
    for text in ("2D1I5=3X4=", "1I2D5=1X2=", "5=1X3=2D1I2D", "2D1I5=1X3=2D1I2D", "1I2D1I5=2X1=3D", "3D5=1X2=1I", "2I1D4=1X2D1I7=3I2D1I"):
        for strand in "+-":
            B.add(_pack(text), {"kind": "quirk", "text": text}, strand=strand)
    B.pad_records(ROWS_MIN_REC + 9)
    return B.finish()


BATCH_NAMES = ("lengths_regular", "lengths_wild", "fate", "route_63_records", "route_64_records", "route_mean_1536", "route_mean_1536_63",
               "route_mean_1537", "defects_5", "defects_300", "defects_2048", "hostile", "magnitude")
WAVE_BATCHES = ("route_63_records", "route_mean_1537")            # the two the wave-per-record kernel takes whole


def batches(seed=0):
    """name -> batch (the dict rbtest_util.batch_args takes, plus `tags`).  Deterministic in `seed`."""
    rng = np.random.default_rng([0x5CA9, seed])
    out = {"lengths_regular": lengths_batch(rng, "regular"), "lengths_wild": lengths_batch(rng, "wild"), "fate": fate_batch(rng)}
    out.update(routing_batches(rng))
    out["defects_5"] = defect_batch(rng, 5)
    out["defects_300"] = defect_batch(rng, 300)
    out["defects_2048"] = defect_batch(rng, 2048, positions=lambda n, head: [0, STEP - head, n - 1])
    out["hostile"] = hostile_batch(rng)
    out["magnitude"] = magnitude_batch(rng)
    return out


def random_short_batch(rng, n_rec, pool=400):
    """n_rec short records drawn from a pool of regular and wild ones of 0..39 words (a few of them empty or below 4 words, which the
    row form lists, and one in a thousand of 2100): the shape the context test grows the scan list with"""
    P = Builder(rng)
    for k in range(pool):
        n = int(rng.integers(0, 40))
        P.add((wild_words if k % 4 == 0 else regular_words)(rng, n), coord="t_en+1" if k % 50 == 7 else "ok")
    P.add(regular_words(rng, 2100))
    p = P.finish()
    idx = rng.integers(0, pool, n_rec)
    idx[rng.random(n_rec) < 0.001] = pool
    out = subset(p, idx)
    out["contig"] = np.zeros(n_rec, np.uint32)
    return out


def subset(b, idx):
    """the records idx of a batch, one behind the other"""
    off = np.asarray(b["op_off"]).astype(np.int64)
    idx = np.asarray(idx, np.int64)
    n = off[idx + 1] - off[idx]
    new = np.zeros(len(idx) + 1, np.uint64)
    new[1:] = np.cumsum(n)
    ops = np.concatenate([b["ops"][off[i]:off[i + 1]] for i in idx]) if len(idx) else np.zeros(0, np.uint32)
    out = dict(ops=ops, op_off=new)
    for k in ("t_st", "t_en", "q_st", "q_en", "strand", "contig"):
        out[k] = np.asarray(b[k])[idx]
    return out


def concat(bs):
    """batches one behind the other"""
    out = dict(ops=np.concatenate([b["ops"] for b in bs]))
    offs, base = [np.zeros(1, np.uint64)], 0
    for b in bs:
        offs.append(np.asarray(b["op_off"][1:], np.uint64) + np.uint64(base))
        base += int(b["op_off"][-1])
    out["op_off"] = np.concatenate(offs)
    for k in ("t_st", "t_en", "q_st", "q_en", "strand", "contig"):
        out[k] = np.concatenate([np.asarray(b[k]) for b in bs])
    return out


def with_long_record(rng, b, mean=ROWS_MEAN_MAX + 1):
    """b with one regular record appended that lifts the batch mean to `mean` ops: the wave-per-record kernel takes the batch"""
    n_rec = len(b["op_off"])                                       # (records after the append)
    need = mean * n_rec - int(b["op_off"][-1])
    w = regular_words(rng, need)
    s = sums(w)
    tail = dict(ops=w, op_off=np.array([0, need], np.uint64), t_st=np.array([10], np.uint64), t_en=np.array([10 + s["R"]], np.uint64),
                q_st=np.array([20], np.uint64), q_en=np.array([20 + s["Q"]], np.uint64), strand=np.array([ord("+")], np.uint8),
                contig=np.zeros(1, np.uint32))
    return concat([b, tail])


# ------------------------------------------------------------------------------------------------ the comparison
def check_flags(red, norm, onorm_status, b, what):
    """flags of every reduce row, and of every norm row whose status is OK, against flags_ref; bit-exact"""
    want_red, want_norm = flags_ref(b)
    bad = np.flatnonzero(red["flags"] != want_red)
    assert len(bad) == 0, f"{what}: reduce.flags differ at {bad[:5]}: {red['flags'][bad[:5]]} vs {want_red[bad[:5]]}"
    ok = np.asarray(onorm_status) == 0
    bad = np.flatnonzero(ok & (norm["flags"] != want_norm))
    assert len(bad) == 0, f"{what}: norm.flags differ at {bad[:5]}: {norm['flags'][bad[:5]]} vs {want_norm[bad[:5]]}"


def check_scan(engine, oracle, b, what, want_route=None):
    """test_gpu_parity._check_scan (every field against the per-base oracle) + the flags of every row + the route the call took
    (want_route: 'rows' / 'wave' / None = whatever route() says)"""
    from rbtest_util import batch_args
    from test_gpu_parity import _check_scan
    red, norm = _check_scan(engine, oracle, b, what)
    got, want = engine.scan_route(), route(b["op_off"])
    assert got == want, f"{what}: the scan took route {got}, the routing rule says {want}"
    if want_route is not None:
        assert (got != (0, 0)) == (want_route == "rows"), f"{what}: expected the {want_route} route, got {got}"
    onorm = oracle.normalize(oracle.Batch(*batch_args(b), b["contig"]))
    check_flags(red, norm, onorm["status"], b, what)
    return red, norm
