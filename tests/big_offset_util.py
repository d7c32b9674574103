"""Byte offsets at and behind 2^32 for the kernels that take 64-bit offsets into one large device buffer (tests/test_gpu_big_offsets.py;
tests/test_big_offset_inputs.py proves, without a GPU, that every case holds what it claims).

INPUTS (rb_dev_parse_cigars, rb_dev_parse_md, rb_dev_bam_records).  A payload is the unchanged output of one of the seam generators
(text_seam_util, sam_util, bam_rec_util): some bytes and the extents of its items in them.  A placement copies the payload to offset K of
a buffer of 2^32 + 16 MiB bytes and moves every input offset by K; K is chosen so that 2^32 falls at a stated place of a stated item.
The reference is the generator's own model on the small payload; only offsets INTO the buffer (md_off, md_end of a BAM record) move.
For K >= 2^32 a decoy lies at K - 2^32: the payload built from the same items rotated, so that an offset that lost its high half reads
well-formed input of another item.

OUTPUTS (rb_dev_format_cigars, rb_dev_nucfreq_text).  More than 4 GiB of text from a small source: a cycle of items / segments repeated,
all repeats sharing their source, so the text is `period` repeated and the model prints one period.  A trimmed variant stops after whole
items so that the text ends on byte 2^32 exactly."""
import struct
from types import SimpleNamespace

import numpy as np

import bam_rec_util as B
import nftext_util as nu
import sam_util as U
import text_seam_util as tu

B32 = 1 << 32
MIB = 1 << 20
TAIL = 16 * MIB
BUF_BYTES = B32 + TAIL
PAST = 4 * MIB                 # the output cases run this far past 2^32 at least
FILL = 0xEE                    # what the buffer holds before every use
K_ABOVE = (B32, B32 + 1, B32 + MIB + 7)   # class (e)
K_SMALL = 4096 + 7             # the placement the CPU companion checks the models' bijection at


# ================================================================================================ payloads
class Payload:
    """kind 'parse' / 'md' / 'bam'; data: the bytes; off / end [n]: the items' extents in data (a BAM record's: rec_off, rec_off +
    rec_len); labels [n]; build(r): the same generator on the items rotated by r"""

    def __init__(self, kind, name, data, off, end, labels, build):
        self.kind, self.name, self.data, self.labels, self._build = kind, name, bytes(data), list(labels), build
        self.off, self.end = np.asarray(off, np.uint64), np.asarray(end, np.uint64)
        self.n = len(self.off)
        self._decoy = None

    def item(self, label):
        return self.labels.index(label)

    def extent(self, i):
        return int(self.off[i]), int(self.end[i])

    def decoy(self):
        """the payload of the same items rotated by DECOY_ROT (one, unless a payload needs another count: see differs_from_decoy)"""
        if self._decoy is None:
            self._decoy = self._build(DECOY_ROT.get((self.kind, self.name), 1))
        return self._decoy

    def same_as_decoy(self):
        """labels of the items that answer the same when their offsets are applied to the decoy (and the buffer's fill behind it), those
        left out that cannot_tell() names"""
        d = self.decoy()
        want = results(self.kind, self.data, self.off, self.end)
        got = results(self.kind, d.data + bytes([FILL]) * max(0, len(self.data) + 64 - len(d.data)), self.off, self.end)
        return [self.labels[i] for i, (a, b, e) in enumerate(zip(want, got, cannot_tell(self))) if a == b and not e]


DECOY_ROT = {("md", "md"): 2, ("bam", "cg"): 2, ("bam", "gather"): 2, ("bam", "status"): 3}   # rotations other than one


def _rot(x, r):
    r %= max(len(x), 1)
    return list(x[r:]) + list(x[:r])


def _parse_payload(name, r=0):
    if r == 0:
        Lo = tu.layout(name)
    else:  # (a Layout keeps its cases' places in the cases themselves: fresh ones, at the phases they asked for)
        fresh = tu.PARSE_LAYOUTS[name]()
        Lo = tu.Layout(name, _rot([tu.Case(c.name, c.s, b0=c.b0 & 15, pin=c.pin, tag=c.tag) for c in fresh.cases], r))
    p = Payload("parse", name, Lo.buffer("paf"), Lo.off, Lo.end, [c.name for c in Lo.cases], lambda rr: _parse_payload(name, rr))
    p.layout = Lo
    return p


def _md_payload(shape, r=0):
    cases = _rot(U.md_cases(shape), r)
    text, off, end = U.md_layout(cases)
    p = Payload("md", "md", text, off, end, [c[0] for c in cases], lambda rr: _md_payload(shape, rr))
    p.strings = [c[1] for c in cases]
    return p


def mixed_cases(shape):
    """the deal of tests/test_gpu_bam_records.py's `mixed`: the case lists dealt into one another, 2049 records and a few more"""
    lists = [B.aux_cases(shape[1]), B.status_cases(), [c for c in B.cg_cases() if c[0] not in ("applies_65536", "applies_70000")], B.field_cases()]
    small = [c for c in B.gather_cases(shape[4]) if len(c[1]) < 400]
    out, k = [], 0
    while len(out) < 2049:
        out.append(small[k % len(small)])
        for ls in lists:
            out.append(ls[k % len(ls)])
        k += 1
    return out


BAM_GROUPS = {"gather": lambda s: B.gather_cases(s[4]), "aux": lambda s: B.aux_cases(s[1]), "cg": lambda s: B.cg_cases(), "status": lambda s: B.status_cases(),
              "fields": lambda s: B.field_cases(), "mixed": mixed_cases}


def _bam_payload(name, shape, r=0, cases=None):
    cases = _rot(BAM_GROUPS[name](shape) if cases is None else cases, r)
    data, off, ln = B.stream([b for _, b in cases])
    p = Payload("bam", name, data, off, off + ln.astype(np.uint64), [lb for lb, _ in cases], lambda rr: _bam_payload(name, shape, rr))
    p.rec_len, p.bodies = ln, [b for _, b in cases]
    return p


_made = {}


def payload(kind, name, shapes):
    """shapes: dict(md=rb_md_shape, bam=rb_bam_shape); built once"""
    key = (kind, name)
    if key not in _made:
        _made[key] = _parse_payload(name) if kind == "parse" else _md_payload(shapes["md"]) if kind == "md" else _bam_payload(name, shapes["bam"])
    return _made[key]


def composition_payload():
    """the records of test_composition_columns_to_rows_equal_the_span_model as a payload (their MDs are real: rb_dev_aln_stats needs them)"""
    import rustybam_amd
    recs = U.span_cases() + list(U.panic_cases().values())
    for i, (label, s, _, _, _) in enumerate(U.md_cases(rustybam_amd.md_shape())):
        k = sum(U.md_host(s.split(b"\0")[0])[:2])
        recs.append(dict(name=f"md{i}", ref=0, pos=1000 + i, flag=16 * (i % 2), l_seq=20, cigar=[(k, "M")] if 0 < k < 2**28 else [(20, "M")], md=s, nm=None))
    data = U.bam_bytes(U.REFS, recs)
    refs, off, ln = B.hop(data)
    p = Payload("bam", "composition", data, off, off + ln.astype(np.uint64), [r["name"] for r in recs], None)
    p.rec_len, p.recs, p.refs = ln, recs, refs
    return p


# ================================================================================================ models
def model(p, K=0, data=None):
    """the generator's own model of payload p, as the call answers when the payload lies at offset K of the buffer.  With data: the model
    of THOSE bytes at p's offsets + K (the bijection check, and what a decoy would answer)"""
    if data is None:  # (computed once on the payload as it is, shared by the tests, never changed: K only moves offsets into the buffer)
        if getattr(p, "_model", None) is None:
            p._model = _model(p, 0, None)
        if p.kind != "bam":
            return p._model
        m = {k: v.copy() for k, v in p._model.items()}
        has = m["has_md"] != 0
        m["md_off"][has] += np.uint64(K)
        m["md_end"][has] += np.uint64(K)
        return m
    return _model(p, K, data)


def _model(p, K, data):
    if p.kind == "parse":
        src = p.data if data is None else data
        at = 0 if data is None else K
        strs = [src[at + a:at + b] for a, b in zip(p.off.tolist(), p.end.tolist())]
        return dict(refs=[tu.ref_parse(s)[0] for s in strs], allowed=[({c.pin} if c.pin is not None and data is None else tu.want_status(s))
                                                                       for c, s in zip(p.layout.cases, strs)])
    if p.kind == "md":
        src = p.data if data is None else data
        at = 0 if data is None else K
        return [U.md_model(src[at + a:at + b]) for a, b in zip(p.off.tolist(), p.end.tolist())]
    if data is None:
        m = B.model(p.data, p.off, p.rec_len)
        has = m["has_md"] != 0
        m["md_off"][has] += np.uint64(K)
        m["md_end"][has] += np.uint64(K)
        return m
    return B.model(data, p.off + np.uint64(K), p.rec_len)


def results(kind, data, off, end):
    """one comparable value per item: what the model says of data[off[i]:end[i]] (a BAM record's offsets relative to the record)"""
    off, end = np.asarray(off, np.uint64), np.asarray(end, np.uint64)
    if kind == "parse":
        return [(None if o is None else tuple(o), tuple(sorted(tu.want_status(data[a:b])))) for a, b in zip(off.tolist(), end.tolist())
                for o in [tu.ref_parse(data[a:b])[0]]]
    if kind == "md":
        return [U.md_model(data[a:b]) for a, b in zip(off.tolist(), end.tolist())]
    m = B.model(data, off, (end - off).astype(np.uint32))
    out = []
    for r in range(len(off)):
        rel = int(off[r]) if m["has_md"][r] else 0
        out.append((int(m["tid"][r]), int(m["pos"][r]), int(m["flag"][r]), int(m["l_seq"][r]), int(m["has_md"][r]), int(m["md_off"][r]) - rel,
                    int(m["md_end"][r]) - rel, int(m["status"][r]), m["ops"][int(m["op_off"][r]):int(m["op_off"][r + 1])].tobytes()))
    return out


def reads_nothing(p):
    """per item: its result depends on no byte of the buffer (an empty string; a record of fewer than 32 bytes: RB_BAM_SHORT_BLOCK)"""
    ln = (p.end - p.off).astype(np.int64)
    return (ln < 32 if p.kind == "bam" else ln == 0).tolist()


def cannot_tell(p):
    """per item: no output of the call can tell the payload's bytes from most others -- it reads nothing, or its answer is a refusal,
    which has one form whatever the bytes are: a string the reference rejects (parse), an MD left to the host (RB_MD_UNUSUAL), a record
    whose status is not RB_BAM_OK"""
    e = reads_nothing(p)
    ext = list(zip(p.off.tolist(), p.end.tolist()))
    if p.kind == "parse":
        return [x or tu.ref_parse(p.data[a:b])[0] is None for x, (a, b) in zip(e, ext)]
    if p.kind == "md":
        return [x or U.md_model(p.data[a:b])[1] != U.MD_OK for x, (a, b) in zip(e, ext)]
    st = B.model(p.data, p.off, p.rec_len)["status"]
    return [x or int(s) != B.BAM_OK for x, s in zip(e, st)]


# ================================================================================================ BAM record anatomy
def anatomy(body):
    """a well-formed record body -> dict(cigar=(at, n words), aux=(start, end), fields=[dict(head, type, value=(a, b), count_at)]): the
    aux walk of bam_rec_util.model, keeping where everything lies (offsets into body)"""
    bs = len(body)
    _, _, l_rn, _, _, n_cig, _, l_seq = struct.unpack_from("<iiBBHHHI", body, 0)
    p = 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    assert p <= bs
    out = dict(cigar=(32 + l_rn, n_cig), aux=(p, bs), fields=[])
    while p + 3 <= bs:
        ty, head = chr(body[p + 2]), p
        p += 3
        f = dict(head=head, tag=body[head:head + 2], type=ty, count_at=None)
        if ty in B.SCALARS:
            f["value"] = (p, p + B.SCALARS[ty])
            p += B.SCALARS[ty]
        elif ty in "ZH":
            q = body.find(b"\0", p)
            q = bs if q < 0 else q
            f["value"] = (p, q)
            p = q + 1
        elif ty == "B":
            if p + 5 > bs:
                break
            cnt = struct.unpack_from("<I", body, p + 1)[0]
            es = B.B_SUB.get(chr(body[p]), 4)
            if p + 5 + es * cnt > bs:
                break
            f["count_at"], f["value"] = p + 1, (p + 5, p + 5 + es * cnt)
            p += 5 + es * cnt
        else:
            break
        out["fields"].append(f)
    return out


# ================================================================================================ placements
# (id, payload, class): what x -- the payload byte that lands on 2^32, K = 2^32 - x -- is, is decided in placement()
PARSE_PLACEMENTS = [("a-row", "status", "a"), ("b-wave", "full-steps", "b"), ("c-first-byte", "splits", "c"), ("d-behind-last", "phases", "d")] + \
    [(f"e{j}-{n}", n, f"e{j}") for n in tu.PARSE_LAYOUTS for j in range(3)] + [(f"f-{n}", n, "f") for n in tu.PARSE_LAYOUTS]
MD_PLACEMENTS = [("a-row", "md", "a"), ("b-wave", "md", "b"), ("c-first-byte", "md", "c"), ("d-behind-last", "md", "d")] + \
    [(f"e{j}", "md", f"e{j}") for j in range(3)] + [("f", "md", "f")]
BAM_PLACEMENTS = [("a-fixed", "fields", "a"), ("a-aux-tag", "aux", "a"), ("a-aux-type", "aux", "a"), ("a-aux-count", "aux", "a"), ("a-z-value", "aux", "a"),
                  ("a-cigar", "gather", "a"), ("b-aux-wave", "aux", "b"), ("b-cg-70000", "cg", "b"), ("c-first-byte", "mixed", "c"),
                  ("d-behind-last", "status", "d")] + \
    [(f"e{j}-{g}", g, f"e{j}") for g in BAM_GROUPS for j in range(3)] + [(f"f-{g}", g, "f") for g in BAM_GROUPS]
PLACEMENTS = {"parse": PARSE_PLACEMENTS, "md": MD_PLACEMENTS, "bam": BAM_PLACEMENTS}
IDS = {k: [x[0] for x in v] for k, v in PLACEMENTS.items()}


def placement(kind, pid, shapes):
    """-> SimpleNamespace(p payload, K, cls, item (index or None), lo, hi: the extent inside the payload of the thing 2^32 lies in / at,
    steps: for class b (byte of the first step's end at the latest, byte of the last step's start at the earliest))"""
    _, name, cls = next(x for x in PLACEMENTS[kind] if x[0] == pid)
    p = payload(kind, name, shapes)
    P = len(p.data)
    out = SimpleNamespace(p=p, cls=cls, item=None, lo=None, hi=None, steps=None, id=pid, kind=kind)
    if cls[0] == "e":
        out.K = K_ABOVE[int(cls[1])]
        return out
    if cls == "f":
        out.K = B32 - P // 2
        return out
    if cls == "d":
        i = p.n - 1
        out.item, x = i, int(p.end[i])
        out.lo, out.hi = p.extent(i)
    elif cls == "c":
        i = p.n // 2 + 1
        while reads_nothing(p)[i]:
            i += 1
        out.item, x = i, int(p.off[i])
        out.lo, out.hi = p.extent(i)
    elif kind == "parse" and cls == "a":
        i = p.item("MM-lane")
        out.item, (out.lo, out.hi) = i, p.extent(i)
        x = (out.lo + out.hi) // 2
    elif kind == "parse" and cls == "b":
        i = max(range(p.n), key=lambda j: int(p.end[j] - p.off[j]))
        out.item, (out.lo, out.hi) = i, p.extent(i)
        a = out.lo & ~15
        x = a + tu.STEP + 16 * 21 + 5          # step 1, lane 21, byte 5
        out.steps = (a + tu.STEP, a + (out.hi - 1 - a) // tu.STEP * tu.STEP)
    elif kind == "md" and cls == "a":
        i = p.item("row_step_split_5_2")
        out.item, (out.lo, out.hi) = i, p.extent(i)
        x = (out.lo + out.hi) // 2
    elif kind == "md" and cls == "b":
        i = p.item("deletion_run_5000")
        out.item, (out.lo, out.hi) = i, p.extent(i)
        x = (out.lo + out.hi) // 2 + 3
        w = shapes["md"][2]
        out.steps = (out.lo + w, out.hi - w)
    else:  # bam a / b: a place inside one record
        label = {"a-fixed": "flag_FFFB", "a-aux-tag": "every_type_in_front", "a-aux-type": "every_type_in_front", "a-aux-count": "every_type_in_front",
                 "a-z-value": "md_len_255", "a-cigar": "gather_65_7_2", "b-aux-wave": "wave_long_Z_then_md", "b-cg-70000": "applies_70000"}[pid]
        i = p.item(label)
        R = int(p.off[i])
        an = anatomy(p.bodies[i])
        out.item = i
        if pid == "a-fixed":
            lo, hi, x = 0, 32, 13
        elif pid in ("a-aux-tag", "a-aux-type", "a-aux-count"):
            f = next(f for f in an["fields"] if f["type"] == "B" and f["tag"] == b"YI")
            lo, hi = f["head"], f["value"][0]          # tag, 'B', subtype, count: eight bytes
            x = {"a-aux-tag": f["head"] + 1, "a-aux-type": f["head"] + 2, "a-aux-count": f["count_at"] + 2}[pid]
        elif pid == "a-z-value":
            f = [f for f in an["fields"] if f["tag"] == b"MD" and f["type"] == "Z"][-1]
            lo, hi = f["value"]
            x = (lo + hi) // 2
        elif pid == "a-cigar":
            lo, hi = an["cigar"][0], an["cigar"][0] + 4 * an["cigar"][1]
            x = lo + 4 * 30 + 2
        elif pid == "b-aux-wave":
            lo, hi = an["aux"]
            x = (lo + hi) // 2 + 1
            out.steps = (lo + shapes["bam"][2], hi - shapes["bam"][2])
        else:
            f = next(f for f in an["fields"] if f["tag"] == b"CG")
            lo, hi = f["value"]
            x = lo + 4 * 35000 + 1
            out.steps = (lo + 4 * shapes["bam"][5], hi - 4 * shapes["bam"][5])
        out.anatomy = an
        out.lo, out.hi, x = R + lo, R + hi, R + x
        if out.steps:
            out.steps = (R + out.steps[0], R + out.steps[1])
    out.x, out.K = x, B32 - x
    return out


# ================================================================================================ periodic output cases
def _u64sum(lens):
    """exclusive prefix [n + 1] of per-item lengths, in uint64"""
    off = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(np.asarray(lens, np.uint64), out=off[1:])
    return off


class Periodic:
    """`reps` repeats of a cycle of `m` items, then `tail` more items (the trimmed variant: a partial cycle and fillers).
    period: the text of one cycle; cyc_len [m]: the cycle's per-item bytes; tail_text / tail_len: of the tail"""

    def n_items(self):
        return self.reps * self.m + len(self.tail_len)

    def item_len(self):
        return np.concatenate([np.tile(np.asarray(self.cyc_len, np.uint64), self.reps), np.asarray(self.tail_len, np.uint64)])

    def text_off(self):
        return _u64sum(self.item_len())

    def total(self):
        return self.reps * len(self.period) + len(self.tail_text)

    def text(self, a, b):
        """bytes [a, b) of the whole text (b - a small)"""
        P, body = len(self.period), self.reps * len(self.period)
        out = bytearray()
        while a < b:
            if a < body:
                k = min(b, body, a - a % P + P)
                out += self.period[a % P:a % P + (k - a)]
            else:
                k = b
                out += self.tail_text[a - body:b - body]
            a = k
        return bytes(out)

    def item_at(self, byte):
        """(item index in the whole call, its extent) of the item that holds text byte `byte`"""
        off = self.text_off()
        i = int(np.searchsorted(off, np.uint64(byte), side="right")) - 1
        return i, int(off[i]), int(off[i + 1])


# ---- rb_dev_nucfreq_text
NF_N = (1000, 256, 257, 4096, 63, 1, 2049, 0)
TEN = (1000000000, 2147483647, 3999999999, 4294967295, 1234567890)


def _nf_table():
    """one small counts table: 4200 positions, every ninth uncovered, counts of 1 - 3 digits with a ten-digit one now and then"""
    rng = np.random.default_rng(41)
    c = rng.integers(0, 700, (4200, 4)).astype(np.uint64)
    k = np.arange(4200)
    for f in range(1, 4):
        sel = k % 11 == f
        c[sel, f] = np.array(TEN, np.uint64)[(k[sel] // 11) % len(TEN)]
    sel = k % 13 == 5
    c[sel, 0] = (1 << 31) - 1 - (k[sel] % 7)      # ten digits in A, below the covered bit
    c[:, 0] |= nu.COVERED
    c[k % 9 == 4, 0] &= nu.COVERED - 1
    return c


def _fix(n, base):
    return bytes(base + (i * 7 + n) % 26 for i in range(n))


def nf_full_cycle(salt=0):
    """the eight segment kinds: n, prefix / suffix lengths (255 / 255 and 0 / 1 among them), seg_cnt into the one table"""
    kinds = []
    fixes = ((6, 4), (255, 255), (0, 1), (16, 17), (1, 15), (255, 0), (15, 16), (3, 3))
    cnts = (0, 100, 3900, 4, 77, 4199, 2100, 50)
    poss = (999000, 9, (1 << 32) - 4096 - 257, 99990 + salt, 0, (1 << 32) - 1, 123456789, 5)
    for n, (pl, sl), cn, ps in zip(NF_N, fixes, cnts, poss):
        kinds.append((cn, ps, n, _fix(pl, 65), _fix(sl, 97)[:-1] + b"\n" if sl else b""))
    return kinds


def _nf_case(mode, table, segs):
    return nu.make_case("big", mode, table, segs)


def _line_lens(case, truth):
    """per-segment bytes of a modelled case"""
    return np.diff(truth[1].astype(np.int64)).tolist()


def _finish(obj, want_inside):
    """reps so that the text passes 2^32 + PAST; the claims the CPU companion re-derives are left to it"""
    P = len(obj.period)
    obj.reps = -(-(B32 + PAST + 1) // P)
    obj.tail_len, obj.tail_text = [], b""
    return obj


def nucfreq_full(trimmed=False):
    """-> Periodic with .case(): the arrays of the whole call.  The salt moves one segment's positions (and so their digit counts)
    until 2^32 lies strictly inside a line of a repeat"""
    key = ("nf-full", trimmed)
    if key in _made:
        return _made[key]
    table = _nf_table()
    for salt in range(0, 4000, 37):
        cyc = nf_full_cycle(salt)
        one = _nf_case(nu.FULL, table, cyc)
        truth = nu.model(one)
        P = len(truth[0])
        r = B32 % P
        if r and r not in set(truth[4]) and r not in set(truth[1].tolist()):
            break
    else:
        raise AssertionError("no salt puts 2^32 inside a line")
    o = Periodic()
    o.kind, o.mode, o.table, o.cycle, o.m, o.period, o.cyc_len, o.one, o.one_truth = "nf", nu.FULL, table, cyc, len(cyc), truth[0], _line_lens(one, truth), one, truth
    _finish(o, True)
    o.tail = []
    if trimmed:
        _nf_trim(o)
    _made[key] = o
    return o


SMALL_N = 4096


def _nf_small_table():
    """4096 + 32 positions: mostly ten-digit counts (a line of about 22 bytes), every 17th position uncovered; behind them rows whose
    line is 4, 5, .. 22 bytes long, for the trimmed variant's last lines"""
    rng = np.random.default_rng(43)
    c = rng.integers(1000000000, 1 << 32, (SMALL_N, 4)).astype(np.uint64)
    k = np.arange(SMALL_N)
    c[k % 5 == 2] = rng.integers(0, 100000, (int((k % 5 == 2).sum()), 4))
    c[:, 0] &= nu.COVERED - 1
    c[:, 0] |= nu.COVERED
    c[k % 17 == 3, 0] &= nu.COVERED - 1
    extra = []
    for ln in range(4, 23):  # nd_a + nd_b + 2 = ln
        na = min(10, ln - 3)
        nb_ = ln - 2 - na
        extra.append([nu.COVERED | (10 ** (na - 1) if na < 10 else 2000000000), 10 ** (nb_ - 1), 0, 0])
    return np.concatenate([c, np.array(extra, np.uint64)])


def nucfreq_small(trimmed=False):
    key = ("nf-small", trimmed)
    if key in _made:
        return _made[key]
    table = _nf_small_table()
    for shift in range(0, 30):   # the cycle: three segments of 4096 positions, the middle one `shift` positions shorter
        cyc = [(0, 1000, SMALL_N, b"", b""), (shift, 77, SMALL_N - shift, b"", b""), (0, 1 << 20, SMALL_N, b"", b"")]
        one = _nf_case(nu.SMALL, table, cyc)
        truth = nu.model(one)
        P = len(truth[0])
        r = B32 % P
        if r and r not in set(truth[4]) and r not in set(truth[1].tolist()):
            break
    else:
        raise AssertionError("no shift puts 2^32 inside a line")
    o = Periodic()
    o.kind, o.mode, o.table, o.cycle, o.m, o.period, o.cyc_len, o.one, o.one_truth = "nf", nu.SMALL, table, cyc, len(cyc), truth[0], _line_lens(one, truth), one, truth
    _finish(o, True)
    o.tail = []
    if trimmed:
        _nf_trim(o)
    _made[key] = o
    return o


def _nf_trim(o):
    """whole cycles, whole segments of the next cycle, then filler segments whose bytes are chosen: the text ends on 2^32"""
    P = len(o.period)
    o.reps = B32 // P
    rest = B32 - o.reps * P
    tail = []
    cyc_off = np.concatenate([[0], np.cumsum(o.cyc_len)]).tolist()
    j = 0
    margin = 1200 if o.mode == nu.FULL else 64
    while j < o.m and cyc_off[j + 1] + margin <= rest:   # whole segments of the cycle
        tail.append(o.cycle[j])
        j += 1
    rest -= cyc_off[j]
    # a run of the table's positions as long as fits, then single lines of chosen length
    seg0 = (0, 4242, 0, b"trim\t", b"\n") if o.mode == nu.FULL else (0, 4242, 0, b"", b"")
    probe = _nf_case(o.mode, o.table, [(0, 4242, min(SMALL_N, len(o.table)), seg0[3], seg0[4])])
    starts = nu.model(probe)[4]
    covered = np.nonzero(o.table[:, 0] & nu.COVERED)[0]
    while True:
        k = 0
        while k + 1 < len(starts) and starts[k + 1] + margin <= rest:
            k += 1
        if not k:
            break
        n = int(covered[k - 1]) + 1            # positions up to and with the k-th covered one: starts[k] bytes
        tail.append((0, 4242, n, seg0[3], seg0[4]))
        rest -= starts[k]
    if o.mode == nu.FULL:
        row, pos = int(covered[0]), 7
        base = len(nu.full_line(b"", pos, int(o.table[row, 0]) & (nu.COVERED - 1), *[int(x) for x in o.table[row, 1:]], b""))
        while rest:
            take = rest if rest <= base + 510 else base + 510 if rest - (base + 510) >= base else rest - base
            assert take >= base
            fix = take - base
            tail.append((row, pos, 1, _fix(min(fix, 255), 65), _fix(fix - min(fix, 255), 97)))
            rest -= take
    else:
        while rest:
            take = rest if rest <= 22 else 22 if rest - 22 >= 4 else rest - 4
            assert 4 <= take <= 22
            tail.append((SMALL_N + take - 4, 7, 1, b"", b""))
            rest -= take
    o.tail = tail
    tc = _nf_case(o.mode, o.table, tail)
    tt = nu.model(tc)
    o.tail_case, o.tail_truth, o.tail_text, o.tail_len = tc, tt, tt[0], _line_lens(tc, tt)


def nf_arrays(o):
    """the whole call: (seg_cnt, seg_pos, seg_n, strings, pre_off, pre_len, suf_off, suf_len, want seg_first, want seg_lines)"""
    cases = [o.one] + ([o.tail_case] if o.tail else [])
    truths = [o.one_truth] + ([o.tail_truth] if o.tail else [])
    blob, cols = b"", []
    for c in cases:
        s, po, pl, so, sl = nu.pack_strings(c)
        cols.append((c.seg_cnt, c.seg_pos, c.seg_n, po + np.uint32(len(blob)), pl, so + np.uint32(len(blob)), sl))
        blob += s
    rep = lambda k: np.concatenate([np.tile(cols[0][k], o.reps)] + [c[k] for c in cols[1:]])  # noqa: E731
    first = np.concatenate([np.tile(truths[0][2], o.reps)] + [t[2] for t in truths[1:]])
    lines = np.concatenate([np.tile(truths[0][3], o.reps)] + [t[3] for t in truths[1:]])
    return SimpleNamespace(seg_cnt=rep(0), seg_pos=rep(1), seg_n=rep(2), strings=blob, pre_off=rep(3), pre_len=rep(4), suf_off=rep(5), suf_len=rep(6),
                           first=first, lines=lines)


# ---- rb_dev_format_cigars
LONG_WORDS = 1000003


def _long_item():
    """about 10^6 words: lengths of one to nine digits (mostly eight and nine), every op code, a continuation pair now and then"""
    k = np.arange(LONG_WORDS, dtype=np.uint64)
    v = (k * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(1 << 28)
    short = k % np.uint64(7) == np.uint64(3)
    v[short] = v[short] % np.uint64(10) ** (np.uint64(1) + k[short] % np.uint64(6))
    v[v == 0] = 1
    w = ((v << np.uint64(4)) | (k % np.uint64(9))).astype(np.uint32)
    for at, val in ((1000, 1 << 28), (500001, 4294967295), (LONG_WORDS - 3, 1000000000)):
        w[at] = tu.word(val, 3)
        w[at + 1] = ((val >> tu.LEN_BITS) << 4) | tu.CONT
    return w


def _format_len_of_words(w):
    """bytes each word of an item prints (a continuation word 0, its owner the digits of the joined length): vectorised, for the long item"""
    w = w.astype(np.uint64)
    ln, code = w >> np.uint64(4), w & np.uint64(15)
    cont = code == tu.CONT
    nxt = np.zeros(len(w), bool)
    nxt[:-1] = cont[1:]
    full = ln.copy()
    full[nxt] += ((w[1:][cont[1:]] >> np.uint64(4)) & np.uint64(15)) << np.uint64(tu.LEN_BITS)
    nd = np.ones(len(w), np.int64)
    for d in range(1, 10):
        nd += full >= np.uint64(10 ** d)
    out = nd + 1
    out[cont] = 0
    return out


def format_case(trimmed=False):
    key = ("fmt", trimmed)
    if key in _made:
        return _made[key]
    sets = [tu.format_seam_items(), tu.format_cont_items(), tu.format_phase_items()]
    long_w = _long_item()
    ops, alt, first, count, fl, ll, base = [], [], [], [], [], [], 0
    for F in sets:
        ops.append(F.ops)
        alt.append(F.alt if F.alt is not None else np.full(len(F.ops), tu.word(77, 8), np.uint32))
        hi = F.first & np.uint64(1 << 63)
        first.append(((F.first & np.uint64((1 << 63) - 1)) + np.uint64(base)) | hi)
        count.append(F.count)
        fl.append(F.fl if F.fl is not None else np.zeros(F.n, np.uint32))
        ll.append(F.ll if F.ll is not None else np.zeros(F.n, np.uint32))
        base += len(F.ops)
    long_first = base
    ops.append(long_w), alt.append(np.full(len(long_w), tu.word(78, 7), np.uint32))
    small_first, small_count, small_fl, small_ll = (np.concatenate(x) for x in (first, count, fl, ll))
    # one-word items of 2 .. 10 bytes, for the trimmed variant's end: words behind the long item
    tune = [tu.word(10 ** (d - 1) + 7 % 10 ** (d - 1) if d > 1 else 7, d % 9) for d in range(1, 10)]
    tune_first = long_first + len(long_w)
    ops.append(np.array(tune, np.uint32)), alt.append(np.full(len(tune), tu.word(79, 6), np.uint32))
    o = Periodic()
    o.kind, o.ops, o.alt, o.long_first, o.tune_first = "fmt", np.concatenate(ops), np.concatenate(alt), long_first, tune_first
    small_text = []
    for F in sets:
        small_text.append([tu.ref_format(F.words(i), *F.clip(i)) for i in range(F.n)])
    small_text = [t for ts in small_text for t in ts]
    long_lens = _format_len_of_words(long_w)
    if "fmt-long" not in _made:
        _made["fmt-long"] = tu.ref_format(long_w)
    long_text = _made["fmt-long"]
    assert len(long_text) == int(long_lens.sum())
    S, L = sum(len(t) for t in small_text), len(long_text)
    assert L > S
    P = S + L
    r = B32 % P
    long_at_front = 0 < r < L
    if long_at_front:
        cyc = [(long_first, LONG_WORDS, 0, 0, long_text)] + [(int(f), int(c), int(a), int(b), t) for f, c, a, b, t in zip(small_first, small_count, small_fl, small_ll, small_text)]
    else:
        cyc = [(int(f), int(c), int(a), int(b), t) for f, c, a, b, t in zip(small_first, small_count, small_fl, small_ll, small_text)] + [(long_first, LONG_WORDS, 0, 0, long_text)]
    o.cycle, o.m = cyc, len(cyc)
    o.period = b"".join(c[4] for c in cyc)
    o.cyc_len = [len(c[4]) for c in cyc]
    o.long_index = 0 if long_at_front else o.m - 1
    _finish(o, True)
    o.tail = []
    if trimmed:
        o.reps = B32 // P
        rest = B32 - o.reps * P
        cyc_off = np.concatenate([[0], np.cumsum(o.cyc_len)]).tolist()
        tail, j = [], 0
        while j < o.m and cyc_off[j + 1] + 64 <= rest:
            tail.append(cyc[j])
            j += 1
        rest -= cyc_off[j]
        wend = np.cumsum(long_lens)              # a piece of the long item (not cut between an owner and its continuation word)
        k = int(np.searchsorted(wend, rest - 64, side="right"))
        while k and (long_w[k - 1] & 15 == tu.CONT or (k < LONG_WORDS and long_w[k] & 15 == tu.CONT)):
            k -= 1
        if k:
            tail.append((long_first, k, 0, 0, tu.ref_format(long_w[:k])))
            rest -= len(tail[-1][4])
        while rest:
            take = rest if rest <= 10 else 10 if rest - 10 >= 2 else rest - 2
            assert 2 <= take <= 10
            wd = tune[take - 2]
            tail.append((tune_first + take - 2, 1, 0, 0, tu.ref_format([wd])))
            assert len(tail[-1][4]) == take
            rest -= take
        o.tail = tail
        o.tail_text, o.tail_len = b"".join(t[4] for t in tail), [len(t[4]) for t in tail]
    _made[key] = o
    return o


def format_arrays(o):
    col = lambda k, dt: np.concatenate([np.tile(np.array([c[k] for c in o.cycle], dt), o.reps), np.array([c[k] for c in o.tail], dt)])  # noqa: E731
    return SimpleNamespace(first=col(0, np.uint64), count=col(1, np.uint32), fl=col(2, np.uint32), ll=col(3, np.uint32))


CAPS = (B32 - 1, B32, B32 + 1, B32 + 15)


# ================================================================================================ one transfer of more than 4 GiB
RING_CHUNK = 32 * MIB          # the staging ring's chunk (include/rustybam_amd.h: rb_dev_upload)
XFER_BYTES = B32 + 64 * MIB
DOWN = (B32 - 32 * MIB, B32 + 32 * MIB)


def xfer_windows():
    """[(start, end)] of the source that hold the pattern, merged and in order; everything else is zero"""
    w = [(0, MIB), (B32 - MIB, B32 + MIB), (XFER_BYTES - 4096, XFER_BYTES)]
    for c in range(0, XFER_BYTES, RING_CHUNK):     # every multiple of the chunk whose +-64 KiB neighbourhood is what is asked for
        if c and abs(c - B32) <= 64 * 1024 + RING_CHUNK * 2:
            w.append((c - 64 * 1024, c + 64 * 1024))
    w.sort()
    out = [w[0]]
    for a, b in w[1:]:
        if a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, min(b, XFER_BYTES)))
    return out


def xfer_pattern(a, b):
    """the source's bytes [a, b) inside a window: a function of the absolute offset with no period that divides a power of two (and never 0
    for long)"""
    k = np.arange(a, b, dtype=np.uint64)
    v = (k * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(56)
    return ((v ^ (k % np.uint64(251))) | np.uint64(1)).astype(np.uint8)
