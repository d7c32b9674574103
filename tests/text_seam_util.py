"""Inputs of the CIGAR text kernels' seam tests (tests/test_text_seam_inputs.py, tests/test_gpu_text_seams.py): case builders aimed at
the boundaries of rb_k_parse_cigars / rb_k_format_cigars (rustybam_amd/csrc/k_text.hip), a plain-Python reference of both operations
(int, str, bytes) and a position model of the parse kernel.  Nothing here is taken from the kernel but its geometry: 16 text bytes per
lane, 64 lanes = 1 KiB per step, counted from the record's start rounded down to 16; the format kernel prints 255 words per step (256
when the item ends in the step) and stores whole 16-byte groups of the output plus a ragged head and tail.

Parse cases are LAYOUTS: strings at chosen absolute offsets of one buffer (text_off + text_end), the bytes between them filled with one
of the FILLS -- what a PAF line has around its CIGAR (`cg:Z:` in front, a tab behind), and bytes chosen to hurt if a mask is one byte
off: digits, op characters, 0xFF.  The buffer ends at the next multiple of 16 behind the last string.  Every layout also has a
back-to-back form (text_end = NULL): the same strings, no gaps, whatever phases that gives.

Status: the reference of a string is its ops or None (rejected) and the lengths of its maximal digit runs; want_status() derives the set
of statuses the device may answer from those alone (include/rustybam_amd.h: RB_TEXT_*; 3 = "a number of ten or more digits, the host's
parser decides" -- never without such a run in a valid string)."""
import numpy as np

OPCH = b"MIDNSHP=X"
CONT = 14                    # continuation word: bits 28.. of the length of the op in front of it
LEN_BITS = 28
OK, BAD, TOO_LONG, UNUSUAL = 0, 1, 2, 3
CHUNK, LANES, STEP = 16, 64, 1024
FMT_STEP = 255               # words a step of the format kernel prints when more than 256 are left
FILLS = ("nine", "letter", "paf", "ff")
MIN_GAP = 6                  # bytes between two strings of a layout at least: room for "\t" and "cg:Z:"


# ------------------------------------------------------------------------------------------------ reference: parse
def ref_parse(s):
    """bytes -> (ops, runs): ops = [(len, code)] or None if CigarString::try_from rejects the string (a u32 in decimal digits, any
    number of leading zeros, then one of MIDNSHP=X; the empty string is the empty CIGAR); runs = lengths of the maximal digit runs"""
    s = bytes(s)
    runs, i, n = [], 0, len(s)
    while i < n:
        if 48 <= s[i] <= 57:
            j = i
            while j < n and 48 <= s[j] <= 57:
                j += 1
            runs.append(j - i)
            i = j
        else:
            i += 1
    ops, i = [], 0
    while i < n:
        j = i
        while j < n and 48 <= s[j] <= 57:
            j += 1
        if j == i or j == n:
            return None, runs
        val, code = int(s[i:j]), OPCH.find(s[j:j + 1])
        if val > 0xFFFFFFFF or code < 0:
            return None, runs
        ops.append((val, code))
        i = j + 1
    return ops, runs


def ref_words(ops):
    """[(len, code)] -> packed words, a length of 2^28 and more as two"""
    out = []
    for ln, code in ops:
        out.append(((ln & ((1 << LEN_BITS) - 1)) << 4) | code)
        if ln >> LEN_BITS:
            out.append(((ln >> LEN_BITS) << 4) | CONT)
    return np.array(out, np.uint32)


def want_status(s):
    """the statuses the device may answer for s, from the reference alone.  No run of ten digits: exactly 0 / 2 for a valid string
    (2: some length >= 2^28), 1 or 3 for a rejected one (3 there: the host's parser rejects it).  With such a run: 3, or 0 with the
    reference's ops for a valid string whose lengths all fit; never 1 or 2 for a valid one"""
    ops, runs = ref_parse(s)
    ten = any(r >= 10 for r in runs)
    if ops is None:
        return {BAD, UNUSUAL}
    big = any(ln >> LEN_BITS for ln, _ in ops)
    if ten:
        return {UNUSUAL} if big else {OK, UNUSUAL}
    return {TOO_LONG} if big else {OK}


# ------------------------------------------------------------------------------------------------ the position model
def place(b0, off):
    """byte `off` of the buffer, in a record that starts at b0 -> (lane, step, byte of its chunk)"""
    rel = off - (b0 & ~15)
    assert rel >= 0
    return rel // CHUNK % LANES, rel // STEP, rel % CHUNK


# ------------------------------------------------------------------------------------------------ layouts
class Case:
    __slots__ = ("name", "s", "b0", "pin", "tag")

    def __init__(self, name, s, b0=None, pin=None, tag=None):
        self.name, self.s, self.b0, self.pin, self.tag = name, bytes(s), b0, pin, tag

    @property
    def b1(self):
        return self.b0 + len(self.s)


def _fill(kind, n, front):
    """n bytes of gap; front: the gap has a string behind it (False: the tail of the buffer)"""
    if kind == "nine":
        return b"9" * n
    if kind == "letter":
        return b"M" * n
    if kind == "ff":
        return b"\xff" * n
    if not front:
        return (b"\t" + b"q" * n)[:n]
    return b"\t" + b"q" * (n - 6) + b"cg:Z:" if n >= 6 else b"\tcg:Z:"[6 - n:]


class Layout:
    """cases at increasing b0 (a case without one gets the first offset of the wanted phase MIN_GAP bytes or more behind its neighbour)"""

    def __init__(self, name, cases, lead=MIN_GAP):
        self.name, self.cases = name, cases
        cur = lead
        for c in cases:
            ph = c.b0
            assert ph is not None and 0 <= ph < 16
            c.b0 = cur + ((ph - cur) & 15)
            cur = c.b1 + MIN_GAP
        last = cases[-1].b1
        self.size = max((last + 15) & ~15, 16)
        self.off = np.array([c.b0 for c in cases], np.uint64)
        self.end = np.array([c.b1 for c in cases], np.uint64)

    def buffer(self, fill):
        out, cur = [], 0
        for c in self.cases:
            out.append(_fill(fill, c.b0 - cur, True))
            out.append(c.s)
            cur = c.b1
        out.append(_fill(fill, self.size - cur, False))
        b = b"".join(out)
        assert len(b) == self.size
        return b

    def back_to_back(self):
        """(buffer, text_off [n + 1]) of the text_end = NULL form"""
        raw = b"".join(c.s for c in self.cases)
        off = np.zeros(len(self.cases) + 1, np.uint64)
        off[1:] = np.cumsum([len(c.s) for c in self.cases])
        size = max((len(raw) + 15) & ~15, 16)
        return raw + b"0" * (size - len(raw)), off

    def expected(self):
        """(ops per case or None, allowed statuses per case)"""
        refs = [ref_parse(c.s)[0] for c in self.cases]
        return refs, [({c.pin} if c.pin is not None else want_status(c.s)) for c in self.cases]


_LEN = [7, 42, 305, 6811, 52094, 1, 99, 100, 9, 123456, 7654321, 10, 88888888, 268435455, 123456789, 3000]


def cigar_of_len(n, seed=0):
    """a valid CIGAR of exactly n bytes (n != 1), lengths of 1 .. 9 digits, every op character"""
    assert n != 1
    out, k = [], seed
    while n:
        d = (1, 2, 1, 3, 5, 1, 2, 9, 4, 1, 7, 2, 6, 8)[k % 14]
        d = min(d, n - 1)
        if n - d - 1 == 1:
            d = d - 1 if d > 1 else d + 1
        v = str(_LEN[(k * 7 + d) % len(_LEN)] * 1000000007 % (10 ** d if d < 9 else 200000000)).rjust(d, "1" if k % 3 else "0")   # (< 2^28)
        out.append(v.encode() + OPCH[k % 9:k % 9 + 1])
        n -= d + 1
        k += 1
    return b"".join(out)


def filler(n, seed=0):
    """n bytes of one-digit ops (n odd: the first one has two digits; n >= 2)"""
    if n == 0:
        return b""
    assert n >= 2
    head = b""
    if n & 1:
        head, n = b"22I", n - 3
    return head + b"".join(b"%d%c" % (1 + (seed + i) % 9, OPCH[(seed + 2 * i) % 9]) for i in range(n // 2))


# family 1: start phase x end phase
def phase_cases():
    cases = []
    for ph in range(16):
        lens = list(range(41)) + [STEP * k - ph + d for k in (1, 2) for d in (-1, 0, 1)]
        for n in lens:
            s = (b"7" if ph % 2 == 0 else b"M") if n == 1 else cigar_of_len(n, seed=ph + n)
            cases.append(Case(f"phase{ph}-len{n}", s, b0=ph, tag=(ph, n)))
    return Layout("phases", cases)


# family 2: every split of every number
SPLIT_VALUES = ["123456789"[:d] for d in range(1, 10)] + ["123456789"[:d].rjust(9, "0") for d in range(1, 9)] + ["268435455"]
SPLIT_PHASES = (0, 1, 15)
SPLIT_BOUNDS = ("lane", "step1", "step2")


def _split_case(v, k, bound, ph, idx):
    lane = (3, 17, 40, 63, 2, 31)[idx % 6]
    B = {"lane": CHUNK * lane, "step1": STEP, "step2": 2 * STEP}[bound]   # from the aligned start
    at = B - k - ph                                                          # where the number starts in the string
    s = filler(at, seed=idx) + v.encode() + OPCH[idx % 9:idx % 9 + 1] + b"3=12X"
    return Case(f"{v}-k{k}-{bound}-ph{ph}", s, b0=ph, tag=(v, k, bound, ph, at, B))


def split_cases(values=SPLIT_VALUES, name="splits"):
    cases, idx = [], 0
    for v in values:
        for k in range(1, len(v) + 1):
            for bound in SPLIT_BOUNDS:
                for ph in SPLIT_PHASES:
                    cases.append(_split_case(v, k, bound, ph, idx))
                    idx += 1
    return Layout(name, cases)


def split_too_long_cases():
    return split_cases(["268435456"], "splits-2^28")


# family 3: full steps
FULL_N = (511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537)


def full_step_cases():
    cases = []
    for ph in (0, 1, 8, 15):
        for n in FULL_N:
            cases.append(Case(f"1M*{n}-ph{ph}", b"1M" * n, b0=ph, tag=(ph, n)))
            cases.append(Case(f"1M2=*{n}-ph{ph}", (b"1M2=" * (n // 2 + 1))[:2 * n], b0=ph, tag=(ph, n)))
    return Layout("full-steps", cases)


def ops_per_step(c):
    """op characters of a (valid) case per step, by the position model"""
    per = {}
    for i, b in enumerate(c.s):
        if b in OPCH:
            st = place(c.b0, c.b0 + i)[1]
            per[st] = per.get(st, 0) + 1
    return [per.get(st, 0) for st in range(max(per) + 1)]


# family 4: all 256 byte values
def byte_cases():
    cases = []
    for b in range(256):
        x = bytes([b])
        for t, (s, pos) in enumerate(((b"5" + x, 1), (x + b"5M", 0), (b"5M" + x + b"M", 2), (b"3=7" + x + b"2X", 3))):
            for par in (0, 1):
                ph = ((par - pos) & 1) + 2 * ((b + t) % 8)   # the byte under test on an even / odd byte, the string at every phase
                cases.append(Case(f"byte{b:02x}-t{t}-par{par}", s, b0=ph, tag=(b, t, par, pos)))
    return Layout("bytes", cases)


# family 5: status at the seams
GOOD = b"5=2X"


def status_cases():
    """every case under test has a good record on both sides"""
    T = []

    def add(name, s, ph=0, pin=None):
        T.append(Case("good", GOOD + OPCH[len(T) % 9:len(T) % 9 + 1].rjust(2, b"4"), b0=(3 * len(T)) % 16))
        T.append(Case(name, s, b0=ph, pin=pin))

    # two op characters in a row across a lane and a step boundary
    add("MM-lane", filler(46) + b"5MM3=", pin=BAD)
    add("MM-step", filler(1022) + b"5MM3=", pin=BAD)
    add("MM-lane-ph15", filler(46 - 15) + b"5MM3=", ph=15, pin=BAD)
    # an op character with no length at byte 0 and byte 15 of the first chunk
    add("M-byte0", b"M5=", ph=0, pin=BAD)
    add("M-byte15", b"M5=", ph=15, pin=BAD)
    # digits alone in the last chunk behind a chunk that ended in digits
    add("tail-digits", filler(14) + b"12345")
    add("tail-digits-step", filler(1022) + b"12345")
    # runs of 9, 10 and 16 digits inside one chunk, across two chunks, across a step
    for nd, v in ((9, b"000000005"), (10, b"0000000012"), (16, b"0000000000000077"), (9, b"268435455"), (10, b"0268435455")):
        for where, at in (("inside", 48 if nd == 16 else 50), ("lanes", 48 - nd // 2), ("step", 1024 - nd // 2), ("step2", 2048 - 1)):
            add(f"run{nd}-{v.decode()}-{where}", filler(at) + v + b"D7=")
            add(f"run{nd}-{v.decode()}-{where}-ph15", filler(at - 15) + v + b"D7=", ph=15)
    # precedence: bad + too long = 1, too long alone = 2, a run of ten digits + anything = 3
    add("bad+long", b"5MM268435456M", pin=BAD)
    add("bad+long-lanes", filler(40) + b"268435456M" + b"MM", pin=BAD)
    add("long", b"268435456M", pin=TOO_LONG)
    add("long-last", b"3=268435456D1=", pin=TOO_LONG)
    add("long-u32max-9digits", b"999999999N", pin=TOO_LONG)
    add("ten+bad", b"0000000001MM", pin=UNUSUAL)
    add("ten+bad-lanes", filler(42) + b"0000000001MM", pin=UNUSUAL)
    add("ten+long", b"3=0268435456M", pin=UNUSUAL)
    add("ten+long+bad", b"3=0268435456MM", pin=UNUSUAL)
    add("ten-u32", b"4294967295M", pin=UNUSUAL)
    add("ten-past-u32", b"4294967296M", pin=UNUSUAL)
    T.append(Case("good", GOOD, b0=9))
    return Layout("status", T)


# family 6: record counts
N_REC = (1, 3, 4, 5, 2047, 2048, 2049, 4097)


def count_cases(n_rec):
    cases = []
    for i in range(n_rec):
        k = 1 + (i * 7 + n_rec) % 3
        s = b"".join(b"%d%c" % (1 + (i * 31 + j * 17) % (9, 99, 999)[(i + j) % 3], OPCH[(i + j) % 9]) for j in range(k))
        cases.append(Case(f"rec{i}", s, b0=(i * 5 + n_rec) % 16))
    return Layout(f"count-{n_rec}", cases)


# ------------------------------------------------------------------------------------------------ reference: format
def ref_format(words, fl=0, ll=0):
    """the words of one item -> its text: <len><op> per op, an op and its continuation word as one length; fl / ll (0 = keep) replace
    the length of the first / last word, a one-word item with both prints fl + ll - len"""
    words = [int(w) for w in words]
    n, out, i = len(words), [], 0
    while i < n:
        ln, code = words[i] >> 4, words[i] & 15
        if n == 1 and fl and ll:
            ln = fl + ll - ln
        elif i == 0 and fl:
            ln = fl
        elif i == n - 1 and ll:
            ln = ll
        if i + 1 < n and words[i + 1] & 15 == CONT:
            ln += ((words[i + 1] >> 4) & 15) << LEN_BITS
            i += 1
        assert code < 9
        out.append(b"%d%c" % (ln, OPCH[code]))
        i += 1
    return b"".join(out)


class FormatSet:
    """items over ops / ops_alt.  first[i] has bit 63 set for an item of ops_alt"""

    def __init__(self, name, ops, alt, first, count, fl=None, ll=None, tags=None):
        self.name = name
        self.ops = np.ascontiguousarray(ops, np.uint32)
        self.alt = None if alt is None else np.ascontiguousarray(alt, np.uint32)
        self.first = np.array(first, np.uint64)
        self.count = np.array(count, np.uint32)
        self.fl = None if fl is None else np.array(fl, np.uint32)
        self.ll = None if ll is None else np.array(ll, np.uint32)
        self.tags = tags
        self.n = len(self.first)

    def words(self, i):
        f = int(self.first[i])
        src = self.alt if f >> 63 else self.ops
        f &= (1 << 63) - 1
        return src[f:f + int(self.count[i])]

    def other_words(self, i):
        f = int(self.first[i])
        src = self.ops if f >> 63 else self.alt
        f &= (1 << 63) - 1
        return src[f:f + int(self.count[i])]

    def clip(self, i):
        return (0 if self.fl is None else int(self.fl[i])), (0 if self.ll is None else int(self.ll[i]))

    def expected(self):
        """(text_off [n + 1], text)"""
        parts = [ref_format(self.words(i), *self.clip(i)) for i in range(self.n)]
        off = np.zeros(self.n + 1, np.uint64)
        off[1:] = np.cumsum([len(p) for p in parts])
        return off, b"".join(parts)


def word(ln, code):
    return ((ln & ((1 << LEN_BITS) - 1)) << 4) | code


def _sizes(nbytes):
    """an item of exactly nbytes bytes of text (2 .. 48): text bytes per op, 2 .. 5 each, 1 .. 12 ops"""
    n = max(-(-nbytes // 5), min(12, nbytes // 2, 1 + nbytes % 5 + nbytes // 7))
    sz = [2] * n
    rem, i = nbytes - 2 * n, 0
    while rem:
        if sz[i % n] < 5:
            sz[i % n] += 1
            rem -= 1
        i += 1
    return sz


def _words_of_sizes(sz, seed):
    return [word((7 * (seed + j) + 3) % 9 * 10 ** (b - 2) + 10 ** (b - 2) + (seed + j) % 10 ** (b - 2), (seed + j) % 9) for j, b in enumerate(sz)]


# family F1: output phase x bytes of the item
F1_PHASES, F1_BYTES = range(16), range(2, 49)


def store_shape(phase, nbytes):
    """how a step of nbytes bytes at output phase `phase` leaves: 'bytes' (no whole 16-byte group), or the groups with 'head', 'tail',
    'both' or neither ('whole'); and the number of whole groups"""
    end = phase + nbytes
    a16, b16 = (phase + 15) & ~15, end & ~15
    if a16 >= b16:
        return "bytes", 0
    head, tail = a16 > phase, end > b16
    return ("both" if head and tail else "head" if head else "tail" if tail else "whole"), (b16 - a16) // 16


def format_phase_items():
    ops, first, count, tags, cur, seed = [], [], [], [], 0, 0
    for ph in F1_PHASES:
        for nb in F1_BYTES:
            sp = (ph - cur) & 15
            if sp < 2:
                sp += 16
            for sz, tag in ((_sizes(sp), None), (_sizes(nb), (ph, nb))):
                w = _words_of_sizes(sz, seed)
                first.append(len(ops))
                count.append(len(w))
                tags.append(tag)
                ops += w
                cur += sum(sz)
                seed += 1
    return FormatSet("phase-x-bytes", ops, None, first, count, tags=tags)


# family F2: the 255-word seam
F2_COUNTS = (1, 2, 4, 5, 254, 255, 256, 257, 510, 511, 512, 766)
F2_MODES = ("first", "last", "both", "neither")


def format_steps(n):
    """[(first word, words printed)] per step of an item of n words"""
    out, i0 = [], 0
    while i0 < n:
        lim = n if n - i0 <= 256 else i0 + FMT_STEP
        out.append((i0, lim - i0))
        i0 = lim
    return out


def format_seam_items():
    ops, first, count, fl, ll, tags = [], [], [], [], [], []
    for n in F2_COUNTS:
        for m, mode in enumerate(F2_MODES):
            first.append(len(ops))
            count.append(n)
            f = 7001 + n + m if mode in ("first", "both") else 0
            for salt in range(16):   # one to three digits; no step of 255 words is a multiple of 16 bytes: the next one starts at another phase
                w = [word(1 + (j * 37 + n + m + salt) % (9 if (j + salt) % 5 else 998), (j + n) % 9) for j in range(n)]
                if all(len(ref_format(w[i0:i0 + k], f if i0 == 0 else 0)) % 16 for i0, k in format_steps(n)[:-1]):
                    break
            ops += w
            fl.append(f)
            ll.append(80001 + n + m if mode in ("last", "both") else 0)
            tags.append((n, mode))
    return FormatSet("255-seam", ops, None, first, count, fl, ll, tags)


# family F3: two source arrays
def format_two_arrays():
    n_words = 1400
    ops = [word(1 + (i * 13) % 977, i % 9) for i in range(n_words)]
    alt = [word(1000 + (i * 29) % 8999, (i + 4) % 9) for i in range(n_words)]
    first, count, tags = [], [], []
    for blk in range(16):                       # the four items of one block: every pattern of the two arrays
        for j in range(4):
            use_alt = (blk >> j) & 1
            i = blk * 4 + j
            f, c = (i * 19) % 1000, (1, 2, 3, 5, 17, 64, 300, 4)[(i + blk) % 8]
            first.append(f | (use_alt << 63))
            count.append(c)
            tags.append(use_alt)
    return FormatSet("two-arrays", ops, alt, first, count, tags=tags)


# family F4: continuation words through both arrays
CONT_VALUES = (1 << 28, 999999999, 1000000000, 4294967295)
CONT_AT = ((300, 3), (300, 254), (300, 255), (300, 256), (300, 298), (255, 253), (256, 254), (257, 255), (258, 256), (2, 0))   # (words of the item, word of the owner)


def format_cont_items():
    ops, alt, first, count, tags = [], [], [], [], []
    k = 0
    for n, at in CONT_AT:
        for v in CONT_VALUES:
            for use_alt in (0, 1):
                w = [word(1 + (j * 11 + k) % 97, (j + k) % 9) for j in range(n)]
                w[at] = word(v, (k + at) % 9)
                w[at + 1] = ((v >> LEN_BITS) << 4) | CONT
                other = [word(500 + (j * 7 + k) % 400, (j + k + 2) % 9) for j in range(n)]
                first.append(len(ops) | (use_alt << 63))
                count.append(n)
                tags.append((n, at, v, use_alt))
                ops += other if use_alt else w
                alt += w if use_alt else other
                k += 1
    # a continuation word in memory directly behind an item's last op: not the item's
    for n in (1, 4, 255, 256, 257):
        for use_alt in (0, 1):
            w = [word(1 + (j * 11 + k) % 97, (j + k) % 9) for j in range(n)] + [(3 << 4) | CONT]
            other = [word(500 + (j * 7 + k) % 400, (j + k + 2) % 9) for j in range(n + 1)]
            first.append(len(ops) | (use_alt << 63))
            count.append(n)
            tags.append((n, None, 0, use_alt))
            ops += other if use_alt else w
            alt += w if use_alt else other
            k += 1
    return FormatSet("continuation", ops, alt, first, count, tags=tags)


# family F5: every digit pattern
TEN_DIGITS = (1000000000, 1000000001, 1010101010, 1098765432, 1234567890, 1999999999, 2000000000, 2147483647, 2147483648, 2718281828,
              2999999999, 3000000000, 3141592653, 3999999999, 4000000000, 4000000001, 4200000000, 4290000000, 4294967294, 4294967295)
F5_ITEM = 1000


def format_digit_values():
    """1 .. 99999, and k * 10000 and k * 10000 + 9999 for every k a packed length has above its four low digits (the last one stops at
    2^28 - 1, the largest length of one word)"""
    v = list(range(1, 100000))
    for k in range(1, 26844):
        v += [k * 10000, min(k * 10000 + 9999, (1 << LEN_BITS) - 1)]
    return v


def format_digit_items():
    vals = format_digit_values()
    ops = ((np.array(vals, np.uint64) << 4) | (np.arange(len(vals), dtype=np.uint64) % 9)).astype(np.uint32)
    pad = (-len(ops)) % F5_ITEM
    ops = np.concatenate([ops, np.full(pad, word(1, 0), np.uint32)])
    tens = []
    for i, t in enumerate(TEN_DIGITS):
        tens += [word(t, i % 9), ((t >> LEN_BITS) << 4) | CONT]
    first = list(range(0, len(ops), F5_ITEM)) + [len(ops)]
    count = [F5_ITEM] * (len(ops) // F5_ITEM) + [len(tens)]
    return FormatSet("digits", np.concatenate([ops, np.array(tens, np.uint32)]), None, first, count)


# ------------------------------------------------------------------------------------------------ the cases, built once
_made = {}
PARSE_LAYOUTS = {"phases": phase_cases, "splits": split_cases, "splits-2^28": split_too_long_cases, "full-steps": full_step_cases,
                 "bytes": byte_cases, "status": status_cases, **{f"count-{n}": (lambda n=n: count_cases(n)) for n in N_REC}}
FORMAT_SETS = {"phase-x-bytes": format_phase_items, "255-seam": format_seam_items, "two-arrays": format_two_arrays,
               "continuation": format_cont_items, "digits": format_digit_items}


def layout(name):
    if name not in _made:
        _made[name] = PARSE_LAYOUTS[name]()
    return _made[name]


def format_set(name):
    if ("f", name) not in _made:
        _made["f", name] = FORMAT_SETS[name]()
    return _made["f", name]
