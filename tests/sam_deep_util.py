"""A deep, irregular record set for `rb stats` on SAM / BAM, shared by test_sam_deep_inputs.py (CPU: the set holds what it claims and the
models agree with the oracle on it), test_gpu_cli_stats_deep.py (files) and test_gpu_aln_stats_deep.py (C ABI).

Records are sam_util's dicts.  Every MD is DERIVED from its CIGAR while the CIGAR is built (_Build): `=` and matched stretches of M add
to a running number; every X base and every chosen mismatch inside an M emits the number and a letter; every D emits the number, '^'
and that many letters; the number is emitted at the end.  So match_count + mismatch_count == diff holds by construction.

The set is built for one shape (bytes per row step, longest string a row takes, bytes per wave step) of rb_k_parse_md; the GPU tests
assert that the library's md_shape() is that shape.  Everything is seeded: two calls give the same records."""
import re

import numpy as np

import sam_util as U

SHAPE = (256, 2048, 1024)
REFS = [("chrA", 2147483647), ("chrB", 5000)]  # (a BAM reference length is an int32)
N_MAPPED = 643                                 # three blocks of rb_k_aln_stats (256 records each); no multiple of 4 or of 256
DECLINE_AT = (130, 300, 511, 600, 642)         # mapped indices of the designed declines: one and more in every block of 256, the last record
N_DECLINES = len(DECLINE_AT)                   # records the device leaves to the host by design (a zero-padded MD number of ten or more digits)
WARN_BEHIND_DECLINE = 131                      # an M-without-MD record directly behind a decline
ON_SECOND_REF = 177
LANE_SCAN = 32                                 # ops between the two ends that a lane of rb_k_aln_stats checks alone; 64 per wavefront step
OP_LENS = (1, 2, 3, 17, 250)
LEADS = ("", "7H", "5S", "7H5S")
TRAILS = ("", "4S", "9H", "4S9H")
BGZF_SIZES = (0xFF00, 1, 4097, 30011, 7, 0xFF00, 65000, 333)  # uncompressed bytes of the BGZF blocks a set is written in: records and lines straddle them


_ACGT = np.frombuffer(b"ACGT", np.uint8)
_ACGTZ = np.frombuffer(b"ACGTZ", np.uint8)
_DIGITS = np.frombuffer(b"0123456789", np.uint8)


class _Build:
    """a CIGAR and the MD that follows from it"""

    def __init__(self, rng):
        self.rng, self.cg, self.md, self.run = rng, [], bytearray(), 0

    def _letters(self, n):
        return _ACGT[self.rng.integers(0, 4, n)].tobytes()

    def _flush(self):
        self.md += b"%d" % self.run
        self.run = 0

    def op(self, ln, c, mism=()):
        """mism: offsets of the mismatches inside an M (ascending)"""
        self.cg.append((int(ln), c))
        if c == "=":
            self.run += ln
        elif c == "M":
            last = 0
            for k in mism:
                self.run += k - last
                self._flush()
                self.md += self._letters(1)
                last = k + 1
            self.run += ln - last
        elif c == "X":
            for _ in range(ln):
                self._flush()
                self.md += self._letters(1)
        elif c == "D":
            self._flush()
            self.md += b"^" + self._letters(ln)
        return self

    def text(self, s):
        for n, c in re.findall(r"(\d+)([MIDNSHP=X])", s):
            self.op(int(n), c)
        return self

    def md_len(self):
        return len(self.md) + len(b"%d" % self.run)

    def finish(self):
        return bytes(self.md) + b"%d" % self.run

    # ---- bodies
    def match(self, mode, ln=None):
        """one op that holds reference and read bases; mode 'M': M only (with mismatches), 'EQ': = / X, 'MIX': all three"""
        rng = self.rng
        ln = OP_LENS[int(rng.integers(5))] if ln is None else ln
        c = "M" if mode == "M" else ("=X"[int(rng.random() < .3)] if mode == "EQ" else "M=X"[int(rng.integers(3))])
        if self.cg and self.cg[-1][1] == c:
            c = {"M": "M", "=": "X", "X": "="}[c]
        if c == "X":
            ln = min(ln, 17)
        mism = sorted(set(int(x) for x in rng.integers(0, ln, int(rng.integers(0, 2 + ln // 8))))) if c == "M" else ()
        return self.op(ln, c, mism)

    def gap(self, pad=.02):
        rng = self.rng
        x = rng.random()
        c = "P" if x < pad else ("N" if x < pad + .03 else "ID"[int(rng.random() < .5)])
        return self.op(OP_LENS[int(rng.integers(4))], c)

    def body(self, mode, n_ops=None, md_len=None, small=False):
        """match (gap match)*: n_ops ops in all (odd), or as many as bring the MD to exactly md_len bytes (mode 'M'; the last op is then an
        M whose mismatches are laid out for it)"""
        self.match(mode, 1 + int(self.rng.integers(3)) if small else None)
        while (len(self.cg) < n_ops) if md_len is None else (self.md_len() < md_len - 600):
            self.gap()
            self.match(mode, 1 + int(self.rng.integers(3)) if small else None)
        if md_len is None:
            return self
        self.op(1, "I")
        at, mism = 0, [0]       # the first mismatch at offset 0 emits the pending number
        left = md_len - (self.md_len() + 1)
        assert left >= 1
        while left > 3:         # a gap of one digit and a letter: two bytes
            at += 1 + int(self.rng.integers(10))
            mism.append(at)
            left -= 2
        tail = int(self.rng.integers(10 ** (left - 1) if left > 1 else 0, 10 ** left))  # a last number of exactly `left` digits
        self.op(at + 1 + tail, "M", mism)
        assert self.md_len() == md_len
        return self


def _finish(b, name, flag=0, lead="", trail="", md=True, seq=True, pos=None, ref=0):
    """the record of a built body between its clips; md False: the tag is left out; seq False: SEQ `*`"""
    cg = [(int(n), c) for n, c in re.findall(r"(\d+)([HS])", lead)] + b.cg + [(int(n), c) for n, c in re.findall(r"(\d+)([HS])", trail)]
    rec = dict(name=name, ref=ref, pos=0, flag=flag, cigar=cg, md=b.finish() if md else None, nm=None)
    rec["l_seq"] = sum(n for n, c in cg if c in "MIS=X") if seq else 0
    t = sum(n for n, c in cg if c in "MDN=X")
    rec["pos"] = int(b.rng.integers(0, REFS[ref][1] - t)) if pos is None else pos
    return rec


def pad_md(md, which=0, width=10):
    """the `which`-th number of the MD written with leading zeros to `width` digits (a negative which counts from the end)"""
    runs = list(re.finditer(rb"\d+", md))
    m = runs[which]
    return md[:m.start()] + m.group().zfill(width) + md[m.end():]


def between_ends(rec):
    """ops between the first op that describes read sequence and the op that holds the last reference base (what rb_k_aln_stats scans)"""
    ops = [c for _, c in rec["cigar"]]
    j = next(i for i, c in enumerate(ops) if c in "MIS=X")
    e = max(i for i, (n, c) in enumerate(rec["cigar"]) if c in "MDN=X" and n)
    return e - j


def situation(rec):
    """which of the four MD situations of bamstats.rs:129-153 the record is in"""
    ops = {c for _, c in rec["cigar"]}
    if "M" not in ops:
        return "no_M"
    if rec["md"] is None:
        return "M_without_MD"
    return "MD_ignored" if "=" in ops else "MD_refines"


def _mapped(shape):
    row_step, row_max, wave_step = shape
    rng = np.random.default_rng(20261021)
    out = []

    def B():
        return _Build(rng)

    def add(rec):
        out.append(rec)

    # A. every combination of clips on both strands, the four MD situations in turn (eight wavefronts of short strings)
    k = 0
    for li, lead in enumerate(LEADS):
        for ti, trail in enumerate(TRAILS):
            for flag in (0, 16):
                mode, md = (("M", True), ("MIX", True), ("M", False), ("EQ", True))[k % 4]
                add(_finish(B().body(mode, 7), f"clip_{li}{ti}_{flag}", flag, lead, trail, md=md))
                k += 1
    # B. a wavefront's four rows with 0, 1, 2, 3 and 4 long strings; records without MD among them
    assert len(out) % 4 == 0
    for c, long_at in enumerate(((), (2,), (0, 3), (0, 1, 3), (0, 1, 2, 3))):
        for slot in range(4):
            if slot in long_at:
                add(_finish(B().body("M", md_len=row_max + 1 + 37 * slot + 500 * c), f"mix{c}_{slot}_long", 16 * (slot & 1), LEADS[slot], TRAILS[c % 4]))
            else:
                add(_finish(B().body("M", 5), f"mix{c}_{slot}_short", 16 * (slot & 1), md=slot != 1))
    # C. MD lengths on both sides of the row / wave threshold and well into the wavefront form
    for n in (row_max - 1, row_max, row_max + 1, 2 * row_max + 1, 3 * wave_step + 1, 3 * wave_step + 17, 3 * wave_step + 500, 4 * wave_step + 3):
        add(_finish(B().body("M", md_len=n), f"md_len_{n}", 16 * (n & 1), LEADS[n % 4], TRAILS[n % 3]))
    # D. ops between the two ends of the span check: a lane alone, one wavefront step, two and more; a pad deep inside
    for n in (1, 31, 33, 63, 65, 127, 129, 301):  # ops of the body; the ends are its first and its last op
        for pad in (False, True):
            b = B().body("EQ" if n % 4 == 1 else "M", n, small=True)
            if pad:
                b.cg.insert(len(b.cg) // 2 + 1, (2, "P"))
            add(_finish(b, f"between_{n}{'_P' if pad else ''}", 16 * pad, LEADS[n % 4], TRAILS[(n // 2) % 4], md=n % 3 != 0))
    # E. what stands behind the last reference base, in front of every trailing clip; an I directly behind the leading clip
    for ti, trail in enumerate(TRAILS):
        for tail in ("2P", "0D", "0N", "3I", "3I2P"):
            add(_finish(B().body("M" if ti % 2 else "EQ", 9).text(tail), f"ends_in_{tail}_{ti}", 16 * (ti & 1), LEADS[ti], trail))
    for li, lead in enumerate(LEADS):
        b = B().op(3, "I")
        add(_finish(b.body("M", 5), f"I_behind_clip_{li}", 16 * (li & 1), lead, TRAILS[li]))
    # F. the bulk: modes, lengths and columns at random; the designed declines at their places
    while len(out) < N_MAPPED:
        i = len(out)
        flag = 16 * int(rng.random() < .5) | (int(rng.random() < .1) << 8)
        lead, trail = LEADS[int(rng.integers(4))], TRAILS[int(rng.integers(4))]
        seq = rng.random() > .15
        if i in DECLINE_AT:
            long_md = i in (300, 642)  # (wavefront form: the padded number sits past the first wave step)
            b = B().body("M", md_len=(3 * wave_step + 77) if long_md else None, n_ops=None if long_md else 21)
            rec = _finish(b, f"decline_{i}", flag, lead, trail, seq=seq)
            rec["md"] = pad_md(rec["md"], which=len(re.findall(rb"\d+", rec["md"])) * 2 // 3 if long_md else (0 if i == 130 else -1), width=10 + i % 3)
        elif i == WARN_BEHIND_DECLINE:
            rec = _finish(B().body("M", 11), f"warn_{i}", flag, lead, trail, md=False)
        elif i == ON_SECOND_REF:
            rec = _finish(B().body("M", 9, small=True), f"second_ref_{i}", flag, lead, trail, ref=1)
        else:
            x = rng.random()
            mode = "M" if x < .55 else ("EQ" if x < .75 else "MIX")
            if mode == "M" and rng.random() < .3:
                b = B().body("M", md_len=int(rng.integers(row_max - 300, 4 * wave_step)))
            else:
                n_ops = int(rng.choice([1, 3, 9, 41, 91, 201, 801, 2401], p=[.1, .2, .25, .2, .1, .08, .05, .02]))
                b = B().body(mode, n_ops, small=n_ops > 100)
            near_end = rng.random() < .1  # a position up to the end of the reference
            rec = _finish(b, f"bulk_{i}", flag, lead, trail, md=rng.random() > (.35 if mode == "M" else .5), seq=seq)
            if near_end:
                rec["pos"] = REFS[0][1] - sum(n for n, c in rec["cigar"] if c in "MDN=X") - int(rng.integers(0, 3))
            if rec["md"] is not None and situation(rec) != "MD_refines" and rng.random() < .1:
                rec["md"] = pad_md(rec["md"], 0, 11)  # a padded number the device never asks about: the MD of a CIGAR with = is ignored
        add(rec)
    assert len(out) == N_MAPPED
    return out, rng


def _unmapped(k, rng):
    star = k % 3 != 0
    return dict(name=f"unmapped_{k}", ref=-1 if star else int(k % 2), pos=-1 if star else int(rng.integers(0, 4000)), flag=4 | (16 if k % 2 else 0) | (64 if k % 5 == 0 else 0),
                l_seq=int(rng.integers(0, 40)), cigar=[], md=None, nm=None)


def _interleave(mapped, rng):
    """unmapped records among the mapped ones (the front drops them: they shift which mapped records share a wavefront of a file's lines)"""
    recs, k = [], 0
    for r in mapped:
        for _ in range(int(rng.random() < .09) + int(rng.random() < .02)):
            recs.append(_unmapped(k, rng))
            k += 1
        recs.append(r)
    return recs


_CACHE = {}


def deep_set(shape=SHAPE):
    """-> (refs, recs): the main set.  Mapped record i of it (unmapped ones not counted) is record i of what the device sees."""
    if shape not in _CACHE:
        mapped, rng = _mapped(shape)
        _CACHE[shape] = _interleave(mapped, rng)
    return REFS, [dict(r) for r in _CACHE[shape]]


def mapped_of(recs):
    return [r for r in recs if not r["flag"] & 4]


def file_index(recs, mapped_index):
    return [i for i, r in enumerate(recs) if not r["flag"] & 4][mapped_index]


PANIC_AT = {"md_disagrees_long": 400, "hardclip_deep": 530, "starts_with_D": 290, "cigar_text": 450, "decline_and_hardclip": 620, "ends_in_D": 515, "ends_in_N": 260}
BAD_CIGAR = b"10=3Q5="


def panic_variants(shape=SHAPE):
    """name -> dict(recs, index (mapped index of the replaced record), sam_edit): the main set with ONE record replaced deep in the file,
    behind records the device leaves to the host and in another block of rb_k_aln_stats than the first.  sam_edit None: the record itself
    panics in the reference (SAM and BAM twin alike); else (old CIGAR text, new): the records are the main set's and the SAM line of
    record `index` gets the malformed CIGAR (a BAM cannot carry it)."""
    row_step, row_max, wave_step = shape
    refs, main = deep_set(shape)
    rng = np.random.default_rng(77)
    out = {}

    def variant(name, rec=None, sam_edit=None):
        recs = [dict(r) for r in main]
        if rec is not None:
            recs[file_index(recs, PANIC_AT[name])] = rec
        out[name] = dict(recs=recs, index=PANIC_AT[name], sam_edit=sam_edit)

    # (a) a long MD, wavefront form, whose counts disagree with the CIGAR by one
    rec = _finish(_Build(rng).body("M", md_len=3 * wave_step + 211), "md_disagrees_long", 16, "7H", "4S")
    tail = re.search(rb"\d+$", rec["md"])
    rec["md"] = rec["md"][:tail.start()] + b"%d" % (int(tail.group()) + 1)
    variant("md_disagrees_long", rec)
    # (b) a hard clip more than 64 ops behind the first end and more than 64 in front of the second
    b = _Build(rng).body("EQ", 161, small=True)
    b.cg.insert(81, (3, "H"))
    variant("hardclip_deep", _finish(b, "hardclip_deep", 0, "5S", "4S9H"))
    # (c) a deletion in front of every op that describes read sequence (M without MD: the reference dies before it would warn)
    b = _Build(rng).op(5, "D")
    variant("starts_with_D", _finish(b.body("M", 9), "starts_with_D", 16, "7H", "", md=False))
    # (d) a CIGAR text the reference's reader dies on: SAM only
    old = main[file_index(main, PANIC_AT["cigar_text"])]
    variant("cigar_text", None, ("".join(f"{n}{c}" for n, c in old["cigar"]).encode(), BAD_CIGAR))
    # (e) a designed decline that is a panic too: a padded MD number and an inner hard clip
    b = _Build(rng).body("M", 41, small=True)
    b.cg.insert(20, (2, "H"))
    rec = _finish(b, "decline_and_hardclip", 0, "5S", "")
    rec["md"] = pad_md(rec["md"], 1, 12)
    variant("decline_and_hardclip", rec)
    # the last reference base inside a D / an N (ahead of trailing clips)
    variant("ends_in_D", _finish(_Build(rng).body("M", 71, small=True).op(5, "D"), "ends_in_D", 16, "", "4S9H"))
    variant("ends_in_N", _finish(_Build(rng).body("EQ", 35, small=True).op(17, "N").op(2, "I"), "ends_in_N", 0, "7H5S", "4S"))
    return out


def variant_sam(refs, v):
    """the SAM text of a panic variant"""
    sam = U.sam_text(refs, v["recs"])
    if v["sam_edit"]:
        old, new = v["sam_edit"]
        name = v["recs"][file_index(v["recs"], v["index"])]["name"].encode()
        at = sam.index(b"\n" + name + b"\t") + 1
        c0 = sam.index(b"\t" + old + b"\t", at)
        assert c0 < sam.index(b"\n", at)
        sam = sam[:c0 + 1] + new + sam[c0 + 1 + len(old):]
    return sam


def sam_with_md_extents(refs, recs):
    """-> (SAM text, md_off, md_end) of the MAPPED records: where every MD value lies in the text (0, 0 without one, as the front passes it)"""
    parts = [U.sam_text(refs, [])]
    at = len(parts[0])
    off, end = [], []
    for r in recs:
        line = U.sam_line(refs, r)
        if not r["flag"] & 4:
            k = line.find(b"\tMD:Z:")
            o = at + k + 6 if k >= 0 else 0
            off.append(o)
            end.append(o + len(r["md"]) if k >= 0 else 0)
        parts.append(line)
        at += len(line)
    return b"".join(parts), np.array(off, np.uint64), np.array(end, np.uint64)


# ------------------------------------------------------------------ line layouts
def layout_sam(refs, recs, md_place="as_is", second_md=False, last="newline"):
    """the SAM text with the MD tag as the 'first', a 'middle' or the 'last' optional field ('cycle': in turn), a second MD:Z: behind
    everything (the first one counts), and the last line ending in a 'newline', in 'nothing' or followed by an 'empty' line"""
    lines = [U.sam_text(refs, [])]
    for i, r in enumerate(recs):
        f = U.sam_line(refs, dict(r, md=None, nm=None)).rstrip(b"\n").split(b"\t")
        opt = [b"AS:i:%d" % (i % 97), b"XS:Z:MD:Z:99", b"NM:i:%d" % (i % 7)]
        if r["md"] is not None:
            place = ("first", "middle", "last")[i % 3] if md_place == "cycle" else md_place
            opt.insert({"first": 0, "middle": 2, "last": 3, "as_is": 3}[place], b"MD:Z:" + r["md"])
            if second_md:
                opt.append(b"MD:Z:%dA7^C" % i)
        if md_place == "as_is" and not second_md:
            opt = opt[3:]
        lines.append(b"\t".join(f + opt) + b"\n")
    text = b"".join(lines)
    return text[:-1] if last == "nothing" else (text + b"\n" if last == "empty" else text)


# ------------------------------------------------------------------ hostile strings for rb_dev_parse_md
N_RANDOM = 2000


def random_md_strings(shape=SHAPE):
    """N_RANDOM strings of 0 .. 2 * row_max + 64 bytes from a hostile alphabet: digits, A-Z, '^', lower case, the bytes next to the three
    classes ('/', ':', '@', '[', ']', '_', '`'), bytes of 0x80 and above; never NUL.  Half of a string is drawn byte by byte, half in
    tokens (numbers of up to twelve digits, letter runs, deletions)."""
    row_step, row_max, wave_step = shape
    rng = np.random.default_rng(4242)
    alphabet = np.array(list(b"0123456789" * 6 + b"ACGTNZAB" * 5 + b"^" * 12 + b"acgtnz" + b"/:@[]_` \t=*" + bytes(range(0x80, 0x100, 9)) + bytes([1, 0x7F, 0xFF])), np.uint8)
    assert 0 not in alphabet
    top = 2 * row_max + 64
    out = []
    for i in range(N_RANDOM):
        x = i % 20
        if i < 4:
            n = (0, 1, top, top - 1)[i]
        elif x < 10:
            n = int(rng.integers(0, 65))
        elif x < 15:
            n = int(rng.integers(65, 2 * row_step + 1))
        elif x < 18:
            n = int(rng.integers(row_max - 64, row_max + 65))
        else:
            n = int(rng.integers(row_max + 1, top + 1))
        s = bytearray()
        while len(s) < n:
            if rng.random() < .5:
                s += alphabet[rng.integers(0, len(alphabet), int(rng.integers(1, 24)))].tobytes()
            else:
                t = rng.random()
                if t < .4:
                    d = int(rng.choice([1, 2, 3, 9, 10, 12], p=[.4, .3, .2, .08, .01, .01]))
                    s += _DIGITS[rng.integers(0, 10, d)].tobytes()
                elif t < .7:
                    s += _ACGT[rng.integers(0, 4, (1, 1, 2, 15, 16, 17, 40)[int(rng.integers(7))])].tobytes()
                else:
                    s += b"^" + _ACGTZ[rng.integers(0, 5, int(rng.choice([0, 1, 2, 5, 16, 33, 300], p=[.05, .3, .3, .2, .1, .04, .01])))].tobytes()
        out.append(bytes(s[:n]))
    return out


def pack_strings(strs, phase=None):
    """-> (text, off, end): the strings back to back with no byte between them (phase None), or every string starting at `phase` modulo
    16 with carets, digits and letters filling up to it"""
    text, off, end = bytearray(), [], []
    for s in strs:
        if phase is not None:
            text += (b"^9Z7A^" * 3)[:(phase - len(text)) % 16]
        off.append(len(text))
        text += s
        end.append(len(text))
    return bytes(text), np.array(off, np.uint64), np.array(end, np.uint64)
