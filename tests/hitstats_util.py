"""Inputs and references of the rb_dev_stats_rows tests (tests/test_gpu_hitstats.py runs them on the device, tests/test_hitstats_inputs.py
proves on the CPU what they hold).

The reference is the ORACLE's reduce row (pyoracle.reduce) of a record that has a hit row's clip -- expanded to plain ops here, in numpy -- as
its CIGAR and the row's coordinates: never the code under test.

  hand_made()    hit rows and an out_ops array built in numpy, no clip kernel in the way: the smallest shapes at which the kernel can go wrong
  real_input()   a synthetic batch, a tenth of it irregular, with its windows: rows and clips as rb_dev_liftover / rb_dev_break leave them"""
import os
import re
from itertools import zip_longest
from types import SimpleNamespace

import numpy as np

import rustybam_amd
from rbtest_util import pack, random_cigar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CODES, QRY_CODES = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)
F_HAS_M = 4
ST_T, ST_Q = 18, 19
GARBAGE = np.uint32((54321 << 4) | 7)  # what lies between the clips: an `=` that would show in every sum
STAT_FIELDS = ("t_bases", "q_bases", "nmatch", "aln_len", "equal", "diff", "ins", "del", "matches", "ins_events", "del_events", "status")
RATIOS = ("id_by_all", "id_by_events", "id_by_matches")


def kernel_shape():
    """(ops per step of a row of 16 lanes, ops per step of a wavefront, longest clip the row form takes): the constants k_hitstats.hip documents"""
    txt = open(os.path.join(ROOT, "rustybam_amd", "csrc", "k_hitstats.hip")).read()
    return tuple(int(re.search(rf"#define {k} (\d+)u", txt).group(1)) for k in ("RB_HS_ROW_STEP", "RB_HS_WAVE_STEP", "RB_HS_ROW_MAX"))


def spans(words):
    """(reference bases, query bases) of packed words, continuation words counted with their owner"""
    w = np.asarray(words, np.uint32).astype(np.uint64)
    code, ln = w & np.uint64(15), w >> np.uint64(4)
    own = code.copy()
    cont = code == 14
    own[cont] = np.roll(code, 1)[cont]
    ln = np.where(cont, (ln & np.uint64(15)) << np.uint64(28), ln)
    return int(ln[np.isin(own, REF_CODES)].sum()), int(ln[np.isin(own, QRY_CODES)].sum())


def expand(h, out_ops, ops, op_off):
    """the clip of hit row h as plain ops (the rules of include/rustybam_amd.h, rb_dev_stats_rows)"""
    off = int(h["out_off"])
    if not int(h["flags"]) & rustybam_amd.HIT_DESCRIPTOR:
        return np.array(out_ops[off:off + int(h["out_n"])], np.uint32)
    d = [int(x) for x in out_ops[off:off + 4]]
    st = int(op_off[int(h["rec"])]) + d[0]
    c = np.array(ops[st:st + d[1]], np.uint32)
    if int(h["flags"]) & rustybam_amd.HIT_INSIDE or len(c) == 0:
        return c
    code = c & np.uint32(15)
    if len(c) == 1 and d[2] and d[3]:
        c[0] = np.uint32(((d[2] + d[3] - (int(c[0]) >> 4)) << 4)) | code[0]
        return c
    if d[2]:
        c[0] = np.uint32(d[2] << 4) | code[0]
    if d[3]:
        c[-1] = np.uint32(d[3] << 4) | code[-1]
    return c


def oracle_stats(oracle, rows, clips):
    """what rb_dev_stats_rows must write for `rows` (either HIT_DT) whose clips, as plain ops, are clips[k] (ignored where the row is not OK):
    the oracle's reduce rows, flags = RB_F_HAS_M where the M lengths of the clip do not sum to 0; all zero but the status where the row is not OK"""
    ok = np.asarray(rows["status"]) == 0
    dense = [np.asarray(c, np.uint32) if o else np.zeros(0, np.uint32) for c, o in zip(clips, ok)]
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in dense])
    b = oracle.Batch(np.concatenate(dense) if dense else np.zeros(0, np.uint32), off, rows["t_st"], rows["t_en"], rows["q_st"], rows["q_en"],
                     np.full(len(rows), ord("+"), np.uint8))
    red = oracle.reduce(b)
    want = np.zeros(len(rows), rustybam_amd.REDUCE_DT)
    for f in STAT_FIELDS + RATIOS:
        want[f] = red[f]
    want["flags"] = [F_HAS_M if o and int((c[(c & 15) == 0] >> 4).sum()) else 0 for c, o in zip(dense, ok)]
    bad = np.nonzero(~ok)[0]
    want[bad] = np.zeros(1, rustybam_amd.REDUCE_DT)
    want["status"][bad] = rows["status"][bad]
    return want


def compare_stats(got, want, what=""):
    """field by field, the three f32 values bitwise"""
    assert len(got) == len(want), f"{what}: {len(got)} stats rows, {len(want)} expected"
    for f in STAT_FIELDS + ("flags",):
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{what}: {f} differs at rows {bad[:6]}: device {got[f][bad[:6]]} oracle {want[f][bad[:6]]}"
    for f in RATIOS:
        bad = np.nonzero(got[f].view(np.uint32) != want[f].view(np.uint32))[0]
        assert len(bad) == 0, f"{what}: {f} differs bitwise at rows {bad[:6]}: device {got[f][bad[:6]]} oracle {want[f][bad[:6]]}"


# ------------------------------------------------------------------------------------------------ 1. hand-made rows
def short_lengths():
    """1, 2, 3 and every value from one below to one above each multiple of a load step, up to two steps, for the row's and the wavefront's step"""
    row_step, wave_step, _ = kernel_shape()
    return sorted({1, 2, 3} | {m * s + d for s in (row_step, wave_step) for m in (1, 2) for d in (-1, 0, 1)})


def long_lengths():
    """clips the wavefront form takes: one op more than the row form's limit, a wavefront's step edge on either side of two multiples, 70,000"""
    _, wave_step, row_max = kernel_shape()
    base = (row_max // wave_step + 1) * wave_step
    return [row_max + 1] + [base + m * wave_step + d for m in (0, 1) for d in (-1, 0, 1)] + [70_000]


def _random_clip(rng, n):
    """n ops of all nine codes (lengths 1 .. 40, a few zero) behind a first op that is an `=`: a clip starts on a match op, so equal + diff is
    never 0 and no ratio is 0 / 0 (the NaN the host's f32 division and the device's may spell differently cannot arise from a clip)"""
    code = rng.choice(9, n, p=[.08, .12, .12, .04, .03, .03, .03, .4, .15]).astype(np.uint32)
    ln = rng.choice([0, 1, 2, 3, 7, 40], n, p=[.02, .42, .2, .16, .15, .05]).astype(np.uint32)
    code[0], ln[0] = 7, max(int(ln[0]), 1)
    return (ln << np.uint32(4)) | code


_hand = None


def hand_made():
    """-> SimpleNamespace(rows HIT_DT, out_ops u32 (its length = the last clip's end rounded up to four words), ops / op_off: the small batch
    the descriptor rows point into, clips: every row's clip as plain ops (None where the row is not OK), kind: what each row is for)"""
    global _hand
    if _hand is not None:
        return _hand
    rng = np.random.default_rng(0x5747)
    row_step, wave_step, row_max = kernel_shape()
    # the small batch of the descriptor rows: regular records of 1, 2, 9, 300 and row_max + 900 ops
    cigs = [random_cigar(rng, n, "regular") for n in (1, 2, 9, 300, row_max + 900)]
    cigs[0] = pack("150=")
    op_off = np.zeros(len(cigs) + 1, np.uint64)
    op_off[1:] = np.cumsum([len(c) for c in cigs])
    ops = np.concatenate(cigs).astype(np.uint32)

    # ---- the items: (kind, words of a plain clip | descriptor (rec, first, count, d2, d3, inside), status, span error) ----
    short = [("short", _random_clip(rng, n), a) for n in short_lengths() for a in range(4)]
    long_ = [("long", _random_clip(rng, n), (i + 1) % 4) for i, n in enumerate(long_lengths())]
    special = [("cont-I", pack("5=300000000I7=2X"), 1), ("cont-EQ", pack("3000000000="), 2), ("cont-EQ", np.concatenate([pack("4=1X3000000000="), pack("9I2=")]), 3),
               ("X-only", pack("17X"), 1), ("M", pack("5M2I3M1D9=4M"), 2), ("M", pack("1M"), 3)]
    for code in range(9):  # every op code on its own behind one `=`
        special.append((f"code{code}", np.array([(1 << 4) | 7, (11 << 4) | code], np.uint32), code % 4))
    GB = 0xDEADBEE
    desc = [("desc-one-both", (0, 0, 1, 100, 120, False)), ("desc-one-first", (0, 0, 1, 77, 0, False)), ("desc-one-last", (0, 0, 1, 0, 33, False)),
            ("desc-one-none", (0, 0, 1, 0, 0, False)), ("desc-multi-both", (3, 5, 120, 1, 1, False)), ("desc-multi-first", (3, 2, 65, 2, 0, False)),
            ("desc-multi-last", (3, 7, 64, 0, 3, False)), ("desc-multi-none", (2, 1, 7, 0, 0, False)), ("desc-two", (1, 0, 2, 1, 1, False)),
            ("desc-inside", (3, 0, 300, GB, GB, True)), ("desc-inside", (0, 0, 1, GB, GB, True)), ("desc-inside", (2, 0, 9, GB, 0, True)),
            ("desc-long", (4, 3, row_max + 700, 1, 1, False)), ("desc-long-inside", (4, 0, row_max + 900, GB, GB, True))]
    desc += [(f"desc-head{a}", (3, 8 + a, 130, 1, 0, False)) for a in range(4)]
    not_ok = [("not-ok", st) for st in (1, 2, 3, 4, 5, 16, 16, 21, 2, 4)]
    wrong = [("wrong-t", _random_clip(rng, 70), 1, "t"), ("wrong-q", _random_clip(rng, 5), 2, "q"), ("wrong-tq", _random_clip(rng, 130), 3, "tq"),
             ("wrong-t-neg", _random_clip(rng, 9), 0, "neg")]

    # short and long, OK and not-OK, plain and descriptor rows side by side in a wavefront's four rows
    order = []
    for group in zip_longest(short, long_, desc, not_ok, special, wrong):
        order += [g for g in group if g is not None]
    order.append(("short-last", _random_clip(rng, 2), 1))  # the last clip ends one word in front of a multiple of four

    rows = np.zeros(len(order), rustybam_amd.HIT_DT)
    out, cur, clips, kinds = [], 0, [], []

    def put(words):
        nonlocal cur
        out.append(np.asarray(words, np.uint32))
        cur += len(words)

    for k, it in enumerate(order):
        kind = it[0]
        kinds.append(kind)
        h = rows[k]
        h["win"] = k
        if kind == "not-ok":
            h["status"], h["out_off"], h["out_n"], h["rec"] = it[1], 0, 7, 0
            h["t_st"], h["t_en"], h["q_st"], h["q_en"] = 5, 9, 1, 2
            clips.append(None)
            continue
        if kind.startswith("desc"):
            rec, first, count, d2, d3, inside = it[1]
            h["rec"], h["out_off"], h["out_n"] = rec, cur, count
            h["flags"] = rustybam_amd.HIT_DESCRIPTOR | (rustybam_amd.HIT_INSIDE if inside else 0)
            put([first, count, d2, d3])
            if k % 3 == 0:
                put([GARBAGE])  # (descriptors at every word offset too)
            c = expand(h, np.concatenate(out), ops, op_off)
        else:
            c, a = np.asarray(it[1], np.uint32), it[2]
            while cur % 4 != a:
                put([GARBAGE])
            h["rec"], h["out_off"], h["out_n"] = k % len(cigs), cur, len(c)
            put(c)
        R, Q = spans(c)
        t_st, q_st = 1000 + 17 * k, 50 + 3 * k
        h["t_st"], h["t_en"], h["q_st"], h["q_en"] = t_st, t_st + R, q_st, q_st + Q
        err = it[3] if len(it) > 3 else None
        if err in ("t", "tq"):
            h["t_en"] += 1
        if err in ("q", "tq"):
            h["q_en"] += 1
        if err == "neg":
            h["t_st"], h["t_en"] = h["t_en"] + 1, h["t_st"]  # t_en < t_st
        clips.append(c)
    while cur % 4:
        put([GARBAGE])
    _hand = SimpleNamespace(rows=rows, out_ops=np.concatenate(out), ops=ops, op_off=op_off, clips=clips, kind=kinds)
    return _hand


# ------------------------------------------------------------------------------------------------ 2. rows from the real kernels
SEED, N_REC = 0x5EED0107, 96
_real = None


def real_input(oracle):
    """96 synthetic records of 150 .. 6000 ops on one contig, both strands, a tenth of them irregular (the generic kernel's), about 40 sliding
    windows and one that strictly contains every record -> SimpleNamespace(b, windows, odd)"""
    global _real
    if _real is not None:
        return _real
    from rustybam_amd import capi
    from rbtest_util import batch_args
    rng = np.random.default_rng(SEED)
    n = capi.synth_n_ops(SEED, 0, N_REC, 150, 6000)
    off = np.zeros(N_REC + 1, np.uint64)
    off[1:] = np.cumsum(n)
    syn = capi.synth_fill_ops_host(SEED, 0, off)
    cigs = [syn[int(off[i]):int(off[i + 1])] for i in range(N_REC)]
    odd = np.zeros(N_REC, bool)
    for i in range(3, N_REC, 10):  # a tenth: irregular CIGARs (all nine codes, zero lengths, adjacent ops of one type; spliced)
        for _ in range(20):
            c = random_cigar(rng, int(rng.integers(150, 2000)), "wild" if (i // 10) % 2 == 0 else "spliced")
            R, Q = spans(c)
            ob = oracle.Batch(c, np.array([0, len(c)], np.uint64), [10], [10 + R], [10], [10 + Q], [ord("+")])
            if oracle.normalize(ob)["status"][0] == 0:  # (records the reference panics on have rows that differ by route)
                cigs[i], odd[i] = c, True
                break
    t_st = np.sort(rng.integers(1000, 60_000, N_REC)).astype(np.uint64)
    q_st = rng.integers(0, 100_000, N_REC).astype(np.uint64)
    sp = np.array([spans(c) for c in cigs], np.uint64)
    b = dict(t_st=t_st, t_en=t_st + sp[:, 0], q_st=q_st, q_en=q_st + sp[:, 1], strand=np.where(np.arange(N_REC) % 2 == 0, ord("+"), ord("-")).astype(np.uint8),
             contig=np.zeros(N_REC, np.uint32))
    b["op_off"] = np.zeros(N_REC + 1, np.uint64)
    b["op_off"][1:] = np.cumsum([len(c) for c in cigs])
    b["ops"] = np.concatenate(cigs).astype(np.uint32)
    hi = int(b["t_en"].max())
    w_st = np.arange(0, hi, hi // 40 + 1, dtype=np.uint64)
    w_en = w_st + np.uint64(hi // 30)
    w_st, w_en = np.append(w_st, np.uint64(0)), np.append(w_en, np.uint64(hi + 10))  # strictly contains every record
    for i in (0, 7, 20, 41, 66):  # a window that is exactly the first deletion of a regular record: rows the reference drops (status 1 .. 5)
        code, ln = cigs[i] & 15, (cigs[i] >> 4).astype(np.uint64)
        j = int(np.nonzero(code == 2)[0][0])
        pos = b["t_st"][i] + ln[:j][np.isin(code[:j], REF_CODES)].sum()
        w_st, w_en = np.append(w_st, pos), np.append(w_en, pos + ln[j])
    order = np.lexsort((w_en, w_st))
    windows = (np.zeros(len(w_st), np.uint32), w_st[order], w_en[order])
    _real = SimpleNamespace(b=b, windows=windows, odd=odd, batch_args=batch_args(b))
    return _real


_real_truth = {}


def real_truth(oracle, legacy=False, max_size=None):
    """the oracle's rows and clips of real_input() (liftover, or break-paf when max_size is given) and the stats rows they must have"""
    key = (bool(legacy), max_size)
    if key not in _real_truth:
        inp = real_input(oracle)
        ob = oracle.Batch(*inp.batch_args, inp.b["contig"])
        pol = oracle.LEGACY if legacy else oracle.MODERN
        rows, ops = oracle.liftover(ob, *inp.windows, policy=pol) if max_size is None else oracle.break_paf(ob, max_size, policy=pol)
        clips = [ops[int(h["out_off"]):int(h["out_off"]) + int(h["out_n"])] if h["status"] == 0 else None for h in rows]
        _real_truth[key] = SimpleNamespace(rows=rows, ops=ops, clips=clips, stats=oracle_stats(oracle, rows, clips))
    return _real_truth[key]
