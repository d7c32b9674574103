"""Inputs and the numpy model of the rb_dev_rows_to_batch tests (tests/test_gpu_rows_to_batch.py runs them on the device,
tests/test_rows_batch_inputs.py proves on the CPU what they hold).

  model()        rows plus out_ops or descriptors in, the dense piece batch out: the contract of include/rustybam_amd.h in numpy, word by word
  hand_made()    hit rows and an out_ops array built in numpy, no clip kernel in the way: the smallest shapes at which the kernel can go wrong
  asm_small()    tests/golden/asm_small.paf as a batch (the rows of rb_dev_break on it are the real-kernel inputs)

The kernel's thresholds are IMPORTED from the library (capi.rows_to_batch_shape -> rb_rows_to_batch_shape, a host function that hands out the
constants k_rows_batch.hip is compiled with), not mirrored: a changed constant moves the inputs with it."""
import os
from types import SimpleNamespace

import numpy as np

import rustybam_amd
from rustybam_amd import capi
from rbtest_util import pack, random_cigar, read_paf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC, INSIDE = rustybam_amd.HIT_DESCRIPTOR, rustybam_amd.HIT_INSIDE
LEN_MASK = 0x0FFFFFFF
GARBAGE = np.uint32((54321 << 4) | 7)  # what lies between the clips
PIECE_FIELDS = ("op_off", "t_st", "t_en", "q_st", "q_en", "strand", "contig", "parent")


def kernel_shape():
    """(ops per step of a row of 16 lanes, longest clip the row form takes, ops per step of a wavefront)"""
    return capi.rows_to_batch_shape()


def clip_words(h, out_ops, ops, op_off):
    """-> (the words of OK row h's clip as rb_dev_rows_to_batch writes them, declined): plain ops are copied as they are; a descriptor's ops
    are copied from the batch with the first / last length replaced (not for INSIDE rows), a one-op clip with both takes d2 + d3 - len; a
    replaced length of 2^28 and more declines and leaves its low 28 bits"""
    off = int(h["out_off"])
    if not int(h["flags"]) & DESC:
        return np.array(out_ops[off:off + int(h["out_n"])], np.uint32), False
    first, count, d2, d3 = (int(x) for x in out_ops[off:off + 4])
    st = int(op_off[int(h["rec"])]) + first
    c = np.array(ops[st:st + count], np.uint32)
    if int(h["flags"]) & INSIDE or count == 0:
        return c, False
    new = {}
    if count == 1 and d2 and d3:
        new[0] = (d2 + d3 - (int(c[0]) >> 4)) & 0xFFFFFFFF
    else:
        if d2:
            new[0] = d2
        if d3:
            new[count - 1] = d3
    declined = False
    for i, ln in new.items():
        declined |= ln > LEN_MASK
        c[i] = np.uint32(((ln & LEN_MASK) << 4) | (int(c[i]) & 15))
    return c, declined


def model(rows, out_ops, ops, op_off, strand, contig):
    """the piece batch of `rows` (HIT_DT): every OK row one piece in row order -> SimpleNamespace(ops, op_off, t_st, t_en, q_st, q_en, strand,
    contig, parent, n_pieces, n_ops, declined)"""
    rows = np.asarray(rows)
    ok = np.nonzero(rows["status"] == 0)[0]
    clips, declined = [], bool((rows["status"] >= 16).any())
    for k in ok:
        c, d = clip_words(rows[k], out_ops, ops, op_off)
        clips.append(c)
        declined |= d
    m = SimpleNamespace(n_pieces=len(ok), declined=declined)
    m.op_off = np.zeros(len(ok) + 1, np.uint64)
    m.op_off[1:] = np.cumsum([len(c) for c in clips])
    m.n_ops = int(m.op_off[-1])
    m.ops = np.concatenate(clips).astype(np.uint32) if clips else np.zeros(0, np.uint32)
    for f in ("t_st", "t_en", "q_st", "q_en"):
        setattr(m, f, rows[f][ok].astype(np.uint64))
    rec = rows["rec"][ok].astype(np.int64)
    m.strand, m.contig = np.asarray(strand, np.uint8)[rec], np.asarray(contig, np.uint32)[rec]
    m.parent = rows["rec"][ok].astype(np.uint32)
    return m


def prefix(m, n_pieces):
    """the model of the first rows that make n_pieces pieces (rows are turned into pieces in order, so a prefix of the rows is a prefix of every array)"""
    p = SimpleNamespace(n_pieces=n_pieces, n_ops=int(m.op_off[n_pieces]), op_off=m.op_off[:n_pieces + 1], ops=m.ops[:int(m.op_off[n_pieces])])
    for f in PIECE_FIELDS[1:]:
        setattr(p, f, getattr(m, f)[:n_pieces])
    return p


# ------------------------------------------------------------------------------------------------ 1. hand-made rows
def threshold_lengths():
    """T - 1, T, T + 1 for every threshold T of the copy kernel: one and two steps of a row (RB_RTB_ROW_STEP), the row / wavefront limit
    (RB_RTB_ROW_MAX), one step of the wavefront (RB_RTB_WAVE_STEP) as a short clip, and -- for clips the wavefront form takes -- the first
    two multiples of its step above the limit"""
    row_step, row_max, wave_step = kernel_shape()
    base = (row_max // wave_step + 1) * wave_step
    ts = [row_step, 2 * row_step, wave_step, row_max, base, base + wave_step]
    return sorted({t + d for t in ts for d in (-1, 0, 1)})


def _random_clip(rng, n):
    """n ops of all nine codes (lengths 1 .. 40, a few zero) behind a first `=`"""
    code = rng.choice(9, n, p=[.08, .12, .12, .04, .03, .03, .03, .4, .15]).astype(np.uint32)
    ln = rng.choice([0, 1, 2, 3, 7, 40], n, p=[.02, .42, .2, .16, .15, .05]).astype(np.uint32)
    code[0], ln[0] = 7, max(int(ln[0]), 1)
    return (ln << np.uint32(4)) | code


_hand = None
BIG = 81_931  # ops of the longest record: its INSIDE descriptor row is the clip of at least 80k ops


def hand_made():
    """-> SimpleNamespace(rows HIT_DT, out_ops u32 (ends with the last clip rounded up to four words), ops / op_off / strand / contig: the small
    batch the descriptor rows point into, kind: what each row is for, src_head: words between the aligned 16-byte group and the clip's first
    word (None where the row is not OK), model: model() of all of it)"""
    global _hand
    if _hand is not None:
        return _hand
    rng = np.random.default_rng(0x0B47C4)
    row_step, row_max, wave_step = kernel_shape()
    cigs = [random_cigar(rng, n, "regular") for n in (1, 2, 9, 300, row_max + 900, BIG)]
    cigs[0] = pack("150=")
    op_off = np.zeros(len(cigs) + 1, np.uint64)
    op_off[1:] = np.cumsum([len(c) for c in cigs])
    ops = np.concatenate(cigs).astype(np.uint32)
    strand = np.array([ord("+"), ord("-"), ord("-"), ord("+"), ord("-"), ord("+")], np.uint8)
    contig = np.array([0, 3, 1, 1, 2, 0], np.uint32)

    # ---- the items: ("plain", words, source offset a, wanted destination offset s or None) | ("desc*", (rec, first, count, d2, d3, inside)) | ("not-ok", status)
    order = []
    short = sorted({1, 2, 3, 4, 5} | {n for n in threshold_lengths() if n <= row_max})
    for n in short:
        for a in range(4):
            for s in (range(4) if n < 4 * row_step else [(a + n) % 4]):  # every (source, destination) word offset for the short clips
                order.append((f"plain{n}", _random_clip(rng, n), a, s))
        order.append(("not-ok", 1 + n % 5))
    GB = 0xDEADBEE
    desc = [("desc-one-both", (0, 0, 1, 100, 120, False)), ("desc-one-first", (0, 0, 1, 77, 0, False)), ("desc-one-last", (0, 0, 1, 0, 33, False)),
            ("desc-one-none", (0, 0, 1, 0, 0, False)), ("desc-multi-both", (3, 5, 120, 1, 1, False)), ("desc-multi-first", (3, 2, 65, 2, 0, False)),
            ("desc-multi-last", (3, 7, 64, 0, 3, False)), ("desc-multi-none", (2, 1, 7, 0, 0, False)), ("desc-two", (1, 0, 2, 1, 1, False)),
            ("desc-inside", (3, 0, 300, GB, GB, True)), ("desc-inside", (0, 0, 1, GB, GB, True)), ("desc-inside", (2, 0, 9, GB, 0, True)),
            ("desc-long", (4, 3, row_max + 700, 1, 1, False)), ("desc-long-inside", (4, 0, row_max + 900, GB, GB, True)),
            ("desc-80k-inside", (5, 0, BIG, GB, GB, True)), ("desc-80k", (5, 1, BIG - 2, 3, 2, False))]
    desc += [(f"desc-head{a}", (3, 8 + a, 130, 1, 0, False)) for a in range(4)]
    desc += [(f"desc-T{n}", (4, 1 + i % 4, n, 2, 1, False)) for i, n in enumerate(n for n in threshold_lengths() if n <= row_max)]
    long_ = [(f"plain{n}", _random_clip(rng, n), i % 4, None) for i, n in enumerate([n for n in threshold_lengths() if n > row_max] + [70_000])]
    special = [("cont-I", pack("5=300000000I7=2X"), 1, None), ("cont-EQ", pack("3000000000="), 2, None), ("M", pack("5M2I3M1D9=4M"), 3, None)]
    tail = []
    for i in range(max(len(desc), len(long_), len(special))):  # long and short, OK and not, plain and descriptor side by side in a wavefront's four rows
        tail += [g[i] for g in (desc, long_, special) if i < len(g)]
        tail.append(("not-ok", 1 + i % 5))
    order = order[:40] + tail + order[40:]
    order.append(("plain-last", _random_clip(rng, 2), 1, None))  # the last clip ends one word in front of a multiple of four

    rows = np.zeros(len(order), rustybam_amd.HIT_DT)
    out, cur, dst, kinds, heads = [], 0, 0, [], []

    def put(words):
        nonlocal cur
        out.append(np.asarray(words, np.uint32))
        cur += len(words)

    fillers = []  # one-op pieces in front of a clip that is to land at a given destination offset
    final_rows = []
    for k, it in enumerate(order):
        kind = it[0]
        h = np.zeros(1, rustybam_amd.HIT_DT)[0]
        h["win"] = k
        t_st, q_st = 1000 + 17 * k, 50 + 3 * k
        h["t_st"], h["t_en"], h["q_st"], h["q_en"] = t_st, t_st + 9 + k % 7, q_st, q_st + 4 + k % 5
        if kind == "not-ok":
            h["status"], h["out_off"], h["out_n"], h["rec"] = it[1], cur, 7, k % len(cigs)
            final_rows.append(h), kinds.append(kind), heads.append(None)
            continue
        if kind.startswith("desc"):
            rec, first, count, d2, d3, inside = it[1]
            if cur % 4 and not kind.startswith("desc-head"):
                while cur % 4:
                    put([GARBAGE])
            h["rec"], h["out_off"], h["out_n"] = rec, cur, count
            h["flags"] = DESC | (INSIDE if inside else 0)
            put([first, count, d2, d3])
            n, head = count, (int(op_off[rec]) + first) % 4
        else:
            c, a, s = np.asarray(it[1], np.uint32), it[2], it[3]
            while s is not None and dst % 4 != s:  # one-op filler pieces until the clip's destination has the wanted word offset
                f = np.zeros(1, rustybam_amd.HIT_DT)[0]
                f["win"], f["rec"], f["out_off"], f["out_n"] = k, 0, cur, 1
                f["t_st"], f["t_en"], f["q_st"], f["q_en"] = 7, 8, 7, 8
                put([(1 << 4) | 7])
                final_rows.append(f), kinds.append("filler"), heads.append((cur - 1) % 4)
                dst += 1
            while cur % 4 != a:
                put([GARBAGE])
            h["rec"], h["out_off"], h["out_n"] = k % len(cigs), cur, len(c)
            put(c)
            n, head = len(c), a
        dst += n
        final_rows.append(h), kinds.append(kind), heads.append(head)
    while cur % 4:
        put([GARBAGE])
    rows = np.array(final_rows, rustybam_amd.HIT_DT)
    out_ops = np.concatenate(out)
    _hand = SimpleNamespace(rows=rows, out_ops=out_ops, ops=ops, op_off=op_off, strand=strand, contig=contig, kind=kinds, src_head=heads,
                            model=model(rows, out_ops, ops, op_off, strand, contig))
    return _hand


def declining():
    """rows that must set info->declined, one set each (on the hand-made batch): -> list of (what, rows, out_ops)"""
    H = hand_made()
    sets = []

    def one(what, status=0, flags=0, desc=None, rec=0):
        rows = np.zeros(3, rustybam_amd.HIT_DT)
        out = [np.array([(5 << 4) | 7, (2 << 4) | 8, GARBAGE, GARBAGE], np.uint32)]
        rows["out_n"], rows["t_en"], rows["q_en"] = 1, 5, 5
        rows["out_off"] = [0, 4, 1]
        rows[1]["status"], rows[1]["flags"], rows[1]["rec"] = status, flags, rec
        d = desc if desc is not None else (0, 1, 0, 0)
        out.append(np.array(d, np.uint32))
        rows[1]["out_n"] = d[1]
        sets.append((what, rows, np.concatenate(out)))

    one("status 16", status=16)
    one("status 22", status=22)
    one("first length 2^28", flags=DESC, desc=(5, 20, 1 << 28, 0), rec=3)
    one("last length 2^28 + 5", flags=DESC, desc=(5, 20, 3, (1 << 28) + 5), rec=3)
    one("one-op clip, d2 + d3 - len = 2^28", flags=DESC, desc=(0, 1, (1 << 28) - 1, 151), rec=0)  # record 0 is 150=
    # and their neighbours that must NOT decline
    one("ok: status 5", status=5)
    one("ok: first length 2^28 - 1", flags=DESC, desc=(5, 20, (1 << 28) - 1, 0), rec=3)
    one("ok: INSIDE row with large d2 / d3", flags=DESC | INSIDE, desc=(5, 20, 1 << 30, 1 << 31), rec=3)
    one("ok: one-op clip, d2 + d3 - len = 2^28 - 1", flags=DESC, desc=(0, 1, (1 << 28) - 1, 150), rec=0)
    return [(w, r, o, model(r, o, H.ops, H.op_off, H.strand, H.contig)) for w, r, o in sets]


# ------------------------------------------------------------------------------------------------ 2. asm_small.paf
_asm = None


def asm_small():
    """tests/golden/asm_small.paf -> dict of the batch's host arrays (DevBatch's argument)"""
    global _asm
    if _asm is None:
        r = read_paf(os.path.join(ROOT, "tests", "golden", "asm_small.paf"))
        _asm = dict(ops=r.ops, op_off=r.op_off, t_st=r.t_st, t_en=r.t_en, q_st=r.q_st, q_en=r.q_en, strand=r.strand, contig=r.contig)
    return _asm


def starts_form(b, rng, gap_max=37):
    """the batch with its records' starts shuffled and gaps between them: op_off becomes a table of starts (RB_LIFT_OP_STARTS form, no [n_rec]
    entry that means anything) -> (ops, op_off); the gaps hold garbage"""
    n = len(b["op_off"]) - 1
    order = rng.permutation(n)
    lens = np.diff(b["op_off"]).astype(np.int64)
    parts, cur, starts = [], 0, np.zeros(n + 1, np.uint64)
    for r in order:
        g = int(rng.integers(0, gap_max))
        parts.append(np.full(g, GARBAGE, np.uint32))
        cur += g
        starts[r] = cur
        parts.append(b["ops"][int(b["op_off"][r]):int(b["op_off"][r + 1])])
        cur += int(lens[r])
    starts[n] = 0  # (never read)
    return np.concatenate(parts).astype(np.uint32), starts
