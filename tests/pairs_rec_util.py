"""`rb orient [--scaffold]` and `rb filter` (paf.rs:91-207, main.rs:234-267) over the RECORDS of a batch as a plain numpy reference -- the
contract of rb_dev_pairs_records / rb_host_pairs_records --, the fabricated inputs of tests/test_gpu_pairs_records.py and
tests/test_pairs_rec_inputs.py, and a writer of the PAF text of a case with the lines the commands print for it.

A record's (t_name, q_name) pair is a dense key.  Per key over the records that take part (key < n_keys): orient = i64 sum of +(q_en - q_st)
on `+` and -(q_en - q_st) on `-`; tspan = sum of w = t_en - t_st; order = sum of (w * (t_st + t_en)) / 2; everything mod 2^64.  key_flip =
orient < 0; key_order = order / tspan (0 where tspan is 0).  Filter: a record passes if q_len > Q and w > A; fspan = sum of w over the records
that pass; kept if it passes and L < fspan.  Every comparison is strict."""
from types import SimpleNamespace

import numpy as np

from rustybam_amd.capi import PAIRS_INFO_DT

ORIENT, FILTER = 1, 2
DECL_KEY, DECL_WRAP, DECL_ZERO_SPAN = 2, 4, 8
U64 = np.uint64
PLUS, MINUS = ord("+"), ord("-")
BIG_Q = 1 << 40  # a q_len no hand-made record ends behind


def case(name, t_st, t_span, q_st, q_span, strand, rec_key, rec_q_len, n_keys, mode=ORIENT | FILTER, L=0, A=0, Q=0, **expect):
    t_st, q_st = np.asarray(t_st, U64), np.asarray(q_st, U64)
    with np.errstate(over="ignore"):
        t_en, q_en = t_st + np.asarray(t_span, U64), q_st + np.asarray(q_span, U64)
    n = len(t_st)
    rec_q_len = np.full(n, rec_q_len, U64) if np.isscalar(rec_q_len) else np.asarray(rec_q_len, U64)
    c = SimpleNamespace(name=name, t_st=t_st, t_en=t_en, q_st=q_st, q_en=q_en, strand=np.asarray(strand, np.uint8), rec_key=np.asarray(rec_key, np.uint32),
                        rec_q_len=rec_q_len, n_keys=int(n_keys), mode=mode, L=int(L), A=int(A), Q=int(Q), expect=expect)
    assert {len(x) for x in columns(c)} == {n}
    return c


def columns(c):
    """the seven input columns in the order of the call's parameter list"""
    return c.t_st, c.t_en, c.q_st, c.q_en, c.strand, c.rec_key, c.rec_q_len


def model(c, mode=None):
    """-> kept (whole: every kept record), q_st / q_en [n_rec], key_flip, key_order, info (for room for all), and the sums the device keeps to
    itself (orient i64, tspan, fspan, order per key; part / keep per record)"""
    mode = c.mode if mode is None else mode
    n, n_keys = len(c.t_st), c.n_keys
    key = c.rec_key.astype(np.int64)
    part = key < n_keys
    declined = DECL_KEY if (~part).any() else 0
    k = key[part]
    orient, tspan, fspan, order = (np.zeros(n_keys, U64) for _ in range(4))
    has = np.zeros(n_keys, bool)
    has[k] = True
    with np.errstate(over="ignore"):
        w, q_span = c.t_en - c.t_st, c.q_en - c.q_st
        passes = (c.rec_q_len > U64(c.Q)) & (w > U64(c.A)) if mode & FILTER else np.ones(n, bool)
        np.add.at(tspan, k, w[part])
        if mode & ORIENT:
            np.add.at(orient, k, np.where(c.strand == MINUS, U64(0) - q_span, q_span)[part])
            np.add.at(order, k, ((w * (c.t_st + c.t_en)) >> U64(1))[part])
        if mode & FILTER:
            np.add.at(fspan, key[part & passes], w[part & passes])
        orient = orient.view(np.int64)
        key_flip = (orient < 0).astype(np.uint8)
        key_order = np.zeros(n_keys, U64)
        nz = (tspan != 0) & bool(mode & ORIENT)
        key_order[nz] = order[nz] // tspan[nz]
        if mode & ORIENT and (has & (tspan == 0)).any():
            declined |= DECL_ZERO_SPAN
        flip = np.zeros(n, bool)
        flip[part] = key_flip[k] != 0
        if (flip & (c.rec_q_len < c.q_en)).any():
            declined |= DECL_WRAP
        q_st = np.where(flip, c.rec_q_len - c.q_en, c.q_st)
        q_en = np.where(flip, c.rec_q_len - c.q_st, c.q_en)
    keep = part & passes
    if mode & FILTER:
        keep[part] &= U64(c.L) < fspan[k]
    kept = np.nonzero(keep)[0].astype(np.uint32)
    info = np.zeros(1, PAIRS_INFO_DT)[0]
    info["n_kept"], info["n_flipped_rows"], info["declined"] = len(kept), int(flip[keep].sum()), declined
    return SimpleNamespace(kept=kept, q_st=q_st, q_en=q_en, key_flip=key_flip, key_order=key_order, info=info, orient=orient, tspan=tspan, fspan=fspan,
                           order=order, part=part, keep=keep, flip=flip, passes=passes)


def model_info(m, kept_cap=None):
    """the info block of a call that is told kept_cap (None: room for all): the counts are exact either way"""
    info = m.info.copy()
    info["overflow"] = 1 if kept_cap is not None and len(m.kept) > kept_cap else 0
    return info


def shape():
    from rustybam_amd.capi import pairs_records_shape
    return pairs_records_shape()


# ------------------------------------------------------------------ fabricated records
def keys_in_runs(n, rng, n_keys, lo=1, hi=20):
    """n keys in runs of random length lo .. hi; neighbouring runs differ"""
    out, last = [], -1
    while len(out) < n:
        k = int(rng.integers(0, n_keys))
        if k == last:
            k = (k + 1) % n_keys
        out += [k] * int(rng.integers(lo, hi + 1))
        last = k
    return np.array(out[:n], np.uint32)


def random_case(n, seed, n_keys=7, mode=ORIENT | FILTER, keys=None, name=None):
    """n records, keys in runs (or `keys`), both strands, a fifth of the queries short; the thresholds cut through the middle of every distribution"""
    rng = np.random.default_rng(seed)
    keys = keys_in_runs(n, rng, n_keys) if keys is None else np.asarray(keys, np.uint32)
    n_keys = max(n_keys, int(keys.max()) + 1 if n else 0) if keys is not None else n_keys
    strand = np.where(rng.random(n) < 0.5, PLUS, MINUS)
    q_len = np.where(rng.random(n) < 0.2, 500, BIG_Q)
    c = case(name or f"random n={n} seed={seed}", rng.integers(0, 1 << 33, n), rng.integers(1, 100, n), rng.integers(0, 400, n), rng.integers(0, 50, n),
             strand, keys, q_len, n_keys, mode, L=0, A=20, Q=500)
    spans = np.sort(model(c, FILTER).fspan)
    c.L = int(spans[len(spans) // 2]) if n else 0  # (the middle key's span: strictly more is kept, so about half the keys go)
    return c


def record_counts():
    """the counts at which a group of 64 lanes, a wavefront's walk (W) and a workgroup (B) of the sum pass fill up, and more than two workgroups"""
    W, B = shape()
    return [0, 1, 63, 64, 65, W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 7]


def run_case(start, run, variant, cut=None):
    """`start` records of key 0, then a run of `run` records of key 1, then 70 of key 2: the run begins at lane start % 64.  Key 1's sums sit
    ON the thresholds, so one record missed or counted twice changes what comes out:
      variant "exact"  orient sum 0 (no flip: one `+` record missed would flip), L = the run's span (dropped: one record twice would keep)
      variant "over"   orient sum -1 (flip: a `+` record counted twice would not), L = span - 1 (kept: one record missed would drop)
    cut: records of the run (offsets into it) whose key is outside the key space -- they count nowhere, the run is cut in two around them."""
    n = start + run + 70
    key = np.concatenate([np.zeros(start), np.ones(run), np.full(70, 2)]).astype(np.uint32)
    strand = np.full(n, PLUS)
    strand[start:start + run][1::2] = MINUS
    strand[start + run:] = MINUS
    if cut is not None:
        key[start + np.asarray(cut)] = 3
    t_span, q_span = np.full(n, 10, np.int64), np.full(n, 4, np.int64)
    live = np.nonzero(key[start:start + run] == 1)[0] + start
    plus, minus = live[strand[live] == PLUS], live[strand[live] == MINUS]
    assert len(plus) and len(minus)
    q_span[plus], q_span[minus] = 6, 0
    q_span[minus[-1]] = 6 * len(plus) + (1 if variant == "over" else 0)
    span = 10 * len(live)
    return case(f"run of {run} at lane {start % 64}, {variant}" + (", cut" if cut is not None else ""), np.arange(n) * 1000 + 7, t_span, np.arange(n) * 10 + 3,
                q_span, strand, key, BIG_Q, 3, L=span if variant == "exact" else span - 1, run=(start, run), flip1=int(variant == "over"),
                kept1=0 if variant == "exact" else len(live), orient1=0 if variant == "exact" else -1, fspan1=span)


def laid_runs_case():
    """runs of 1 .. 130 records, each on another key than its neighbours, cut so that a run ends at lane 62, at lane 63 (on a group boundary), at
    lane 0, on a wavefront's and on a workgroup's boundary -- and begins there, since the next run follows at once.  The keys come round again
    (41 of them), so the wavefronts of several workgroups add to one key."""
    W, B = shape()
    n = 2 * B + 300
    ends = {63, 64, 65, 127, 128, 129, W - 1, W, W + 1, W + 64, 2 * W, B - 1, B, B + 1, B + 63, B + 64, B + 65, B + W, 2 * B, 2 * B + 1, n}  # a run ends in front of each
    rng = np.random.default_rng(62)
    cuts, at, longest = [], 0, False
    for e in sorted(ends):
        while e - at > 130:
            at += int(rng.integers(1, 131)) if longest else 130
            longest = True
            cuts.append(at)
        if e > at:
            cuts.append(e)
            at = e
    lens = np.diff([0] + cuts)
    assert lens.min() >= 1 and lens.max() <= 130 and cuts[-1] == n
    keys = np.repeat(np.arange(len(lens)) % 41, lens)
    c = random_case(n, 62, n_keys=41, keys=keys, name="runs of 1 .. 130 laid on the seams")
    c.expect = dict(cuts=cuts)
    return c


def layout_cases():
    W, B = shape()
    out = [run_case(start, run, v) for run in (63, 64, 65, 129, 130) for start in (0, 1, 63) for v in ("exact", "over")]
    out += [run_case(5, 130, v, cut=[0, 40, 41, 64, 128]) for v in ("exact", "over")]
    for v in ("exact", "over"):  # one key for all records: a wavefront's open run is carried, and the other wavefronts add to the same key
        c = run_case(0, W + 700, v)
        n = W + 700
        for k, a in vars(c).items():
            if isinstance(a, np.ndarray):
                setattr(c, k, a[:n].copy())
        c.name = f"one key, {v}"
        out.append(c)
    n = 300
    out.append(random_case(n, 4, keys=np.arange(n), name="every record its own key"))
    c = random_case(B + 100, 5, keys=np.arange(B + 100) % 2, name="two keys alternating")
    out.append(c)
    out.append(laid_runs_case())
    return out


def threshold_cases():
    """every strict comparison from both sides"""
    out = []
    for name, minus_q, flip in (("orient sum 0", 30, 0), ("orient sum -1", 31, 1), ("orient sum +1", 29, 0)):
        out.append(case(name, [0, 100, 200, 300], [10] * 4, [0, 10, 20, 60], [10, 10, minus_q, 10], [PLUS, PLUS, MINUS, PLUS], [0] * 4, BIG_Q, 1, mode=ORIENT,
                        key_flip=[flip], orient=[30 - minus_q]))
    t3 = ([0, 100, 200], [10, 20, 30], [0, 10, 20], [1, 1, 1], [PLUS] * 3, [0] * 3)
    out.append(case("fspan == L", *t3, BIG_Q, 1, L=60, kept=0))
    out.append(case("fspan == L + 1", *t3, BIG_Q, 1, L=59, kept=3))
    out.append(case("span == A and A + 1", [0, 100, 200], [19, 20, 21], [0, 10, 20], [1, 1, 1], [PLUS] * 3, [0] * 3, BIG_Q, 1, A=20, kept=1))
    out.append(case("q_len == Q and Q + 1", [0, 100, 200], [10] * 3, [0, 10, 20], [1, 1, 1], [PLUS] * 3, [0] * 3, [99, 100, 101], 1, Q=100, kept=1))
    # a record that fails A / Q does not count in fspan -- 10 + 20 + 30 with the 10 out leaves 50, under L = 55 -- yet counts in orient: it is the one
    # `-` record, and its 40 query bases flip the key
    out.append(case("a record that fails A counts in orient only", [0, 100, 200], [10, 20, 30], [0, 50, 70], [40, 9, 9], [MINUS, PLUS, PLUS], [0] * 3, BIG_Q, 1,
                    L=55, A=10, kept=0, key_flip=[1], fspan=[50], tspan=[60]))
    out.append(case("a record that fails Q counts in orient only", [0, 100, 200], [10, 20, 30], [0, 50, 70], [40, 9, 9], [MINUS, PLUS, PLUS], [0] * 3,
                    [5, 1000, 1000], 1, L=55, Q=5, kept=0, key_flip=[1], fspan=[50], tspan=[60]))
    out.append(case("defaults drop q_len == 0 and span 0", [0, 100, 200], [10, 10, 0], [0, 0, 0], [0, 0, 1], [PLUS] * 3, [0] * 3, [0, 7, 7], 1, mode=FILTER, kept=1))
    return out


def wide_cases():
    """spans of 2^62: the sums and the order product leave 64 bits"""
    H = 1 << 62
    out = []
    # tspan = 5 * 2^62 = 2^62 mod 2^64; order: each product wraps; orient = 3 * 2^62 on `+` is -2^62 as an i64: flipped
    out.append(case("spans of 2^62: five records", [3, H + 1, 7, H + 5, 11], [H] * 5, [0, 1, 2, 3, 4], [H, H, H, 5, 5], [PLUS] * 5, [0] * 5, 1 << 63, 1,
                    mode=ORIENT, key_flip=[1], tspan=[H], orient=[3 * H + 10 - (1 << 64)]))
    out.append(case("spans of 2^62: the filter's sum wraps under L", [3, H + 1, 7, H + 5, 11], [H] * 5, [0, 1, 2, 3, 4], [1] * 5, [PLUS] * 5, [0] * 5, 1 << 63, 1,
                    mode=FILTER, L=H, kept=0, fspan=[H]))
    out.append(case("spans of 2^62: four make a span of 0", [3, H + 1, 7, H + 5], [H] * 4, [0, 1, 2, 3], [1] * 4, [PLUS] * 4, [0] * 4, 1 << 63, 1, mode=ORIENT,
                    declined=DECL_ZERO_SPAN, tspan=[0]))
    return out


def mode_cases():
    base = random_case(500, 77)
    out = []
    for name, mode in (("neither", 0), ("orient only", ORIENT), ("filter only", FILTER), ("both", ORIENT | FILTER)):
        c = SimpleNamespace(**vars(base))
        c.name, c.mode = f"mode {mode}: {name}", mode
        out.append(c)
    return out


def decline_cases():
    """each reason alone, the other records of the call well-formed (and what comes out is still the model's)"""
    out = []
    c = random_case(200, 9)
    c.rec_key[130] = c.n_keys
    c.name, c.expect = "declines: a key == n_keys", dict(declined=DECL_KEY)
    out.append(c)
    c = random_case(200, 9)
    c.rec_key[0] = 0xFFFFFFFF
    c.name, c.expect = "declines: key 0xFFFFFFFF", dict(declined=DECL_KEY)
    out.append(c)
    w = ([0, 100, 200], [10, 10, 10], [0, 100, 10], [5, 5, 50], [PLUS, PLUS, MINUS], [0, 0, 0])
    out.append(case("declines: q_len < q_en under a flip", *w, [104, 104, 1000], 1, mode=ORIENT, declined=DECL_WRAP, key_flip=[1]))
    out.append(case("does not decline: q_len == q_en under a flip", *w, [105, 105, 1000], 1, mode=ORIENT, declined=0, key_flip=[1]))
    z = ([0, 50, 50, 100], [10, 0, 0, 10], [0, 10, 20, 30], [5, 5, 5, 5], [PLUS] * 4, [0, 1, 1, 0])
    out.append(case("declines: a key whose target span is 0", *z, BIG_Q, 3, mode=ORIENT, declined=DECL_ZERO_SPAN))
    out.append(case("does not decline: span 0 without orient", *z, BIG_Q, 3, mode=FILTER, declined=0))
    return out


def all_cases():
    out = [random_case(n, 100 + n) for n in record_counts()]
    return out + layout_cases() + threshold_cases() + wide_cases() + mode_cases() + decline_cases()


# ------------------------------------------------------------------ a case as PAF text, and what the commands print for it
def text_case(name, recs, mode=ORIENT, L=0, A=0, Q=0, insert=0, **expect):
    """recs: (q_name, q_len, q_st, q_span, strand, t_name, t_len, t_st, t_span) per record"""
    from pairs_util import intern_pairs
    q_name, q_len, q_st, q_span, strand, t_name, t_len, t_st, t_span = zip(*recs)
    key, n_keys = intern_pairs(t_name, q_name)
    c = case(name, t_st, t_span, q_st, q_span, [ord(s) for s in strand], key, q_len, n_keys, mode, L, A, Q, **expect)
    c.q_name, c.t_name, c.t_len, c.insert = list(q_name), list(t_name), list(t_len), insert
    return c


def cigar_of(t_span, q_span, salt=0):
    """(cg:Z: value, nmatch, aln_len) of a CIGAR in `=` / `X` / `I` / `D` that consumes exactly the two spans"""
    a = min(t_span, q_span)
    x = a // 3 if salt % 2 else 0
    parts = [(a - x - (a - x) // 2, "="), (t_span - a, "D"), (x, "X"), (q_span - a, "I"), ((a - x) // 2, "=")]
    parts = [(k, o) for k, o in parts if k]
    assert parts, "a record with no base has no CIGAR to write"
    return "".join(f"{k}{o}" for k, o in parts), a, sum(k for k, _ in parts)  # (nmatch counts `=` and `X`: paf.rs:631-654)


def paf_text(c, sep="\t", tags=("tp:A:P",)):
    """the case as PAF lines: twelve columns (nmatch, aln_len and mapq not what comes out: Paf::from_file overwrites the first two), tags, cg:Z:"""
    lines = []
    for r in range(len(c.t_st)):
        cg, _, _ = cigar_of(int(c.t_en[r] - c.t_st[r]), int(c.q_en[r] - c.q_st[r]), r)
        cols = [c.q_name[r], int(c.rec_q_len[r]), int(c.q_st[r]), int(c.q_en[r]), chr(c.strand[r]), c.t_name[r], c.t_len[r], int(c.t_st[r]), int(c.t_en[r]), 1, 2,
                30 + r % 31, *tags[:r % (len(tags) + 1)], f"cg:Z:{cg}", *tags[r % (len(tags) + 1):]]
        lines.append(sep.join(map(str, cols)) + "\n")
    return "".join(lines).encode()


def lines_of(c, m, scaffold=False):
    """what `rb orient [--scaffold -i c.insert]` (c.mode == ORIENT) or `rb filter` (FILTER) prints for the text case c, from the model's outputs"""
    orient = bool(c.mode & ORIENT)
    q_st, q_en = [int(x) for x in m.q_st], [int(x) for x in m.q_en]
    q_name = [nm + (("-" if m.flip[r] else "+") if orient else "") for r, nm in enumerate(c.q_name)]
    q_len = [int(x) for x in c.rec_q_len]
    order = [int(r) for r in m.kept]
    if scaffold:  # paf.rs:160-207 on the oriented records
        order.sort(key=lambda r: (c.t_name[r].encode(), int(m.key_order[c.rec_key[r]]), q_st[r]))  # (list.sort is stable)
        i = 0
        while i < len(order):
            j = i
            while j < len(order) and c.t_name[order[j]] == c.t_name[order[i]]:
                j += 1
            names, length, a = [], 0, i
            while a < j:
                b = a
                while b < j and q_name[order[b]] == q_name[order[a]]:
                    b += 1
                if q_name[order[a]] not in names:
                    names.append(q_name[order[a]])
                lo, hi = min(q_st[r] for r in order[a:b]), max(q_en[r] for r in order[a:b])
                for r in order[a:b]:
                    q_st[r], q_en[r] = q_st[r] - lo + length, q_en[r] - lo + length
                length += hi - lo + c.insert
                a = b
            length -= c.insert
            for r in order[i:j]:
                q_name[r], q_len[r] = "::".join(names), length
            i = j
    out = []
    for r in order:
        cg, nmatch, aln_len = cigar_of(int(c.t_en[r] - c.t_st[r]), int(c.q_en[r] - c.q_st[r]), r)
        s = chr(c.strand[r])
        if m.flip[r]:
            s = "-" if s == "+" else "+"
        out.append("\t".join(map(str, [q_name[r], q_len[r], q_st[r], q_en[r], s, c.t_name[r], c.t_len[r], int(c.t_st[r]), int(c.t_en[r]), nmatch, aln_len,
                                       30 + r % 31, "id:Z:", f"cg:Z:{cg}"])) + "\n")
    return "".join(out).encode()


def text_cases():
    R = []
    # T1: qa flipped (two `-` records outweigh one `+`), qb unflipped, qz with an orient sum of exactly 0 (not flipped)
    R += [("qa", 1000, 10, 40, "-", "T1", 9000, 100, 40), ("qa", 1000, 100, 30, "+", "T1", 9000, 200, 33), ("qa", 1000, 200, 45, "-", "T1", 9000, 300, 41)]
    R += [("qb", 800, 0, 50, "+", "T1", 9000, 1000, 50), ("qb", 800, 60, 20, "-", "T1", 9000, 1100, 25)]
    R += [("qz", 500, 0, 20, "+", "T1", 9000, 2000, 20), ("qz", 500, 30, 20, "-", "T1", 9000, 2030, 20)]
    # T0 (sorts in front of T1, appears behind it): qc and qd with the same order (the same target intervals), so --scaffold falls back on q_st'
    # and their records interleave: runs qc, qd, qc, qd
    R += [("qc", 600, 0, 10, "+", "T0", 7000, 100, 10), ("qd", 700, 5, 10, "+", "T0", 7000, 100, 10), ("qc", 600, 20, 10, "+", "T0", 7000, 300, 10),
          ("qd", 700, 25, 10, "+", "T0", 7000, 300, 10)]
    # qa again on another target: another pair, not flipped there
    R += [("qa", 1000, 500, 60, "+", "T0", 7000, 5000, 66)]
    return R


def orient_text_cases():
    R = text_cases()
    return [text_case("orient, insert 0", R, insert=0), text_case("orient, insert 1000000", R, insert=1000000), text_case("orient, insert 7", R, insert=7)]


def filter_text_cases():
    R = text_cases()
    # what each filter drops: qshort by --query, the 20- and 25-base records by --aln, and by --paired-len the pairs left with 40 + 33 + 41 = 114
    # bases and less (qa on T1 is dropped at 114 and kept at 113; its 33-base record goes first at --aln 33, leaving 81); qshort and qlong have 200
    R += [("qshort", 100, 0, 90, "+", "T1", 9000, 4000, 200), ("qlong", 101, 0, 90, "+", "T1", 9000, 5000, 200)]
    out = [text_case("filter defaults", R, mode=FILTER), text_case("filter --query 100", R, mode=FILTER, Q=100), text_case("filter --aln 25", R, mode=FILTER, A=25),
           text_case("filter --paired-len 114", R, mode=FILTER, L=114), text_case("filter --paired-len 113", R, mode=FILTER, L=113),
           text_case("filter -p 81 -a 33 -q 100", R, mode=FILTER, L=81, A=33, Q=100), text_case("filter -p 80 -a 33 -q 100", R, mode=FILTER, L=80, A=33, Q=100)]
    return out


def filter_flags(c):
    return [x for k, v in (("--paired-len", c.L), ("--aln", c.A), ("--query", c.Q)) if v for x in (k, v)]
