"""Shared by the SAM stats tests: alignment records as dicts -> BAM bytes / SAM text, a golden BAM -> the same dicts, and plain-Python
models of the MD rules (rb_dev_parse_md) and of the span rules (rb_dev_aln_stats) with the stats lines that follow from them.

A record is dict(name, ref (index into refs, -1: unmapped), pos (0-based), flag, l_seq, cigar [(len, op char)], md (bytes or None),
nm (int or None)).  refs is [(name, length)].  The models know nothing of the product's code: test_sam_inputs.py holds them to the oracle."""
import gzip
import struct
import zlib

import numpy as np

OPCH = "MIDNSHP=X"
MD_OK, MD_UNUSUAL = 0, 3
ALN_OK, ALN_DEL_FIRST, ALN_HARDCLIP, ALN_NONE, ALN_MD_ASSERT, ALN_MD_STATUS = 0, 32, 33, 34, 35, 64
ALN_WARN_M = 1
U32 = 0xFFFFFFFF

ALN_DT = np.dtype([("r_en", "<i8"), ("q_st", "<i8"), ("q_en", "<i8"), ("q_len", "<i8"), ("equal", "<u4"), ("diff", "<u4"), ("ins", "<u4"),
                   ("del", "<u4"), ("matches", "<u4"), ("ins_events", "<u4"), ("del_events", "<u4"), ("id_by_all", "<f4"),
                   ("id_by_events", "<f4"), ("id_by_matches", "<f4"), ("status", "<u4"), ("flags", "<u4")])
assert ALN_DT.itemsize == 80


# ------------------------------------------------------------------ the MD rules
def _md_counts(s):
    s = bytes(s)
    m = mm = ic = ib = 0
    unusual = False
    i, n = 0, len(s)
    while i < n:
        c = s[i]
        if 48 <= c <= 57 or 65 <= c <= 90:
            j = i
            while j < n and (48 <= s[j] <= 57) == (48 <= c <= 57) and (65 <= s[j] <= 90) == (65 <= c <= 90):
                j += 1
            if 48 <= c <= 57:  # a maximal digit run adds its value
                unusual = unusual or j - i >= 10
                m += int(s[i:j])
            elif i > 0 and s[i - 1] == 94:  # a maximal run of A-Z behind '^': one deletion event
                ic += 1
                ib += j - i
            else:  # every other A-Z byte: one mismatch
                mm += j - i
            i = j
        else:
            i += 1
    return (m & U32, mm & U32, ic & U32, ib & U32), unusual


def md_model(s):
    """-> ((match_count, mismatch_count, deletion events, deletion bases), status): the regex (\\d+)|([A-Z])|(\\^[A-Z]+) left to right, as
    runs.  Sums wrap in u32.  A digit run of ten or more digits: MD_UNUSUAL and four zeros (the device leaves the string to the host)."""
    out, unusual = _md_counts(s)
    return ((0, 0, 0, 0), MD_UNUSUAL) if unusual else (out, MD_OK)


def md_host(s):
    """the counts whatever the digit runs look like (the host's parse_md_for_stats)"""
    return _md_counts(s)[0]


# ------------------------------------------------------------------ the span rules
def _f32_ratios(equal, diff, ins, dele, ins_ev, del_ev):
    with np.errstate(divide="ignore", invalid="ignore"):
        num = np.float32(100.0) * np.float32(np.uint32(equal))
        return tuple(num / np.float32(np.uint32(d & U32)) for d in (equal + diff + dele + ins, equal + diff + del_ev + ins_ev, equal + diff))


def counters(cigar):
    """what the record scan counts: dict(t_bases, q_bases, equal, diff, ins, del, matches, ins_events, del_events) (u32 counters wrap)"""
    L = {c: 0 for c in OPCH}
    ev = {"I": 0, "D": 0}
    for ln, c in cigar:
        L[c] += ln
        if c in ev:
            ev[c] += 1
    return dict(t_bases=sum(L[c] for c in "MDN=X"), q_bases=sum(L[c] for c in "MIS=X"), equal=L["="] & U32, diff=(L["X"] + L["M"]) & U32,
                ins=L["I"] & U32, **{"del": L["D"] & U32}, matches=L["M"] & U32, ins_events=ev["I"], del_events=ev["D"])


def span_model(rec, md4=None, md_status=MD_OK):
    """-> one ALN_DT row for the record.  md4 / md_status: what rb_dev_parse_md gave for rec['md'] (default: md_model of it)."""
    row = np.zeros(1, ALN_DT)[0]
    cg = rec["cigar"]
    c = counters(cg)
    ops = [o for _, o in cg]
    # rust-htslib CigarStringView::read_pos(end_pos - 1, false, false), walked from the left as the library does
    n, status, qpos = len(ops), None, 0
    j = 0
    for i, o in enumerate(ops):
        if o in "MX=IS":
            j = i
            break
        if o in "DN":
            status = ALN_DEL_FIRST  # 'deletion' found before any operation describing read sequence
            break
        if o == "H" and 0 < i < n - 1:
            status = ALN_HARDCLIP  # hard clip between operations
            break
        if i == n - 1:  # H / P to the end
            status = ALN_NONE
    if n == 0 or (status is None and c["t_bases"] == 0):
        status = ALN_NONE
    if status is None:
        left, status = c["t_bases"] - 1, ALN_NONE  # reference bases in front of the last one; None unless an M / = / X holds it
        while j < n:
            ln, o = cg[j]
            if o in "M=X":
                if left < ln:
                    qpos, status = qpos + left, ALN_OK
                    break
                left -= ln
                qpos += ln
            elif o in "SI":
                qpos += ln
            elif o in "DN":
                if left < ln:
                    break  # the base is deleted from the read
                left -= ln
            elif o == "H":
                status = ALN_HARDCLIP
                break
            j += 1
    if status != ALN_OK:
        row["status"] = status
        return row
    lead_h = cg[0][0] if ops[0] == "H" else 0
    lead_s = cg[0][0] if ops[0] == "S" else (cg[1][0] if len(ops) > 1 and ops[0] == "H" and ops[1] == "S" else 0)
    trail_h = cg[-1][0] if ops[-1] == "H" else 0
    q_st, q_en = lead_h + lead_s, lead_h + 1 + qpos
    q_len = lead_h + rec["l_seq"] + trail_h
    if rec["flag"] & 16:
        q_st, q_en = q_len - q_en, q_len - q_st
    equal, diff, flags = c["equal"], c["diff"], 0
    has_md = rec.get("md") is not None
    if equal == 0 and c["matches"] > 0 and has_md:
        if md4 is None:
            md4, md_status = md_model(rec["md"])
        if md_status != MD_OK:
            row["status"] = ALN_MD_STATUS | md_status
            return row
        if (md4[0] + md4[1]) & U32 != diff:
            row["status"] = ALN_MD_ASSERT
            return row
        equal, diff = md4[0], md4[1]
    elif c["matches"] > 0 and not has_md:
        flags |= ALN_WARN_M
    row["r_en"], row["q_st"], row["q_en"], row["q_len"] = rec["pos"] + c["t_bases"], q_st, q_en, q_len
    row["equal"], row["diff"] = equal, diff
    for k in ("ins", "del", "matches", "ins_events", "del_events"):
        row[k] = c[k]
    row["id_by_all"], row["id_by_events"], row["id_by_matches"] = _f32_ratios(equal, diff, c["ins"], c["del"], c["ins_events"], c["del_events"])
    row["flags"] = flags
    return row


def f32_display(v):
    """Rust's Display of an f32"""
    v = np.float32(v)
    if np.isnan(v):
        return "NaN"
    if np.isinf(v):
        return "inf" if v > 0 else "-inf"
    return np.format_float_positional(v, unique=True, trim="-")


HEADER = {False: "#reference_name\treference_start\treference_end\treference_length\tstrand\tquery_name\tquery_start\tquery_end\tquery_length\t",
          True: "#query_name\tquery_start\tquery_end\tquery_length\tstrand\treference_name\treference_start\treference_end\treference_length\t"}
HEADER_TAIL = "perID_by_matches\tperID_by_events\tperID_by_all\tmatches\tmismatches\tdeletion_events\tinsertion_events\tdeletions\tinsertions\n"


def stats_model(refs, recs, qbed):
    """-> (stdout bytes, exit code) of `rb stats [--qbed]` on the records: the header, one line per mapped record, and 101 at the first
    record whose row is a panic (the lines before it stay).  An unusual MD is recomputed by md_host, as the host does."""
    out = [HEADER[qbed] + HEADER_TAIL]
    for rec in recs:
        if rec["flag"] & 4:
            continue
        row = span_model(rec)
        if row["status"] == (ALN_MD_STATUS | MD_UNUSUAL):
            row = span_model(rec, md_host(rec["md"]), MD_OK)
        if row["status"] != ALN_OK:
            return "".join(out).encode(), 101
        r = [refs[rec["ref"]][0], rec["pos"], int(row["r_en"]), refs[rec["ref"]][1]]
        q = [rec["name"], int(row["q_st"]), int(row["q_en"]), int(row["q_len"])]
        a, b = (q, r) if qbed else (r, q)
        f = a + ["-" if rec["flag"] & 16 else "+"] + b
        f += [f32_display(row["id_by_matches"]), f32_display(row["id_by_events"]), f32_display(row["id_by_all"])]
        f += [int(row[k]) for k in ("equal", "diff", "del_events", "ins_events", "del", "ins")]
        out.append("\t".join(map(str, f)) + "\n")
    return "".join(out).encode(), 0


# ------------------------------------------------------------------ records -> BAM bytes / SAM text
def _aux(rec):
    aux = b""
    if rec.get("md") is not None:
        aux += b"MDZ" + bytes(rec["md"]) + b"\0"
    if rec.get("nm") is not None:
        aux += b"NMi" + struct.pack("<i", rec["nm"])
    return aux


def bam_bytes(refs, recs):
    """the uncompressed BAM stream of the records"""
    out = bytearray(b"BAM\x01")
    text = b"@HD\tVN:1.6\n"
    out += struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for nm, ln in refs:
        out += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    for r in recs:
        name = r["name"].encode() + b"\0"
        cig = b"".join(struct.pack("<I", (ln << 4) | OPCH.index(c)) for ln, c in r["cigar"])
        l_seq = r["l_seq"]
        body = struct.pack("<iiBBHHHiiii", r["ref"], r["pos"], len(name), 60, 0, len(r["cigar"]), r["flag"], l_seq, -1, -1, 0)
        body += name + cig + b"\xff" * ((l_seq + 1) // 2) + b"\xff" * l_seq + _aux(r)  # (SEQ all N, no qualities)
        out += struct.pack("<i", len(body)) + body
    return bytes(out)


def write_bam(path, refs, recs):
    with gzip.open(path, "wb", compresslevel=1) as f:
        f.write(bam_bytes(refs, recs))


def bgzf_bytes(data, sizes=(0xFF00,)):
    """the data as BGZF blocks (SAM spec 4.1: gzip members that carry their own size in a BC subfield) of the given uncompressed sizes in
    turn, and the empty end-of-file block"""
    out, at, k = bytearray(), 0, 0
    while True:
        chunk = data[at:at + sizes[k % len(sizes)]]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = co.compress(chunk) + co.flush()
        assert len(body) + 26 <= 0x10000
        out += struct.pack("<4BI2BH2BHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(body) + 25) + body + struct.pack("<II", zlib.crc32(chunk), len(chunk))
        if not chunk:
            return bytes(out)
        at, k = at + len(chunk), k + 1


def sam_line(refs, r):
    mapped = r["ref"] >= 0
    cg = "".join(f"{ln}{c}" for ln, c in r["cigar"]) or "*"
    f = [r["name"], r["flag"], refs[r["ref"]][0] if mapped else "*", r["pos"] + 1, 60, cg, "*", 0, 0, "N" * r["l_seq"] or "*", "*"]
    line = "\t".join(map(str, f)).encode()
    if r.get("md") is not None:
        line += b"\tMD:Z:" + bytes(r["md"])
    if r.get("nm") is not None:
        line += b"\tNM:i:%d" % r["nm"]
    return line + b"\n"


def sam_text(refs, recs, header=True):
    """SEQ is l_seq x N, QUAL *, aux MD:Z: / NM:i:"""
    out = [b"@HD\tVN:1.6\tSO:unsorted\n"] + [b"@SQ\tSN:%s\tLN:%d\n" % (nm.encode(), ln) for nm, ln in refs] if header else []
    return b"".join(out + [sam_line(refs, r) for r in recs])


# ------------------------------------------------------------------ a golden BAM -> (refs, recs)
def read_bam(path):
    raw = gzip.decompress(open(path, "rb").read())
    assert raw[:4] == b"BAM\x01"
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", raw, p)[0]
        refs.append((raw[p + 4:p + 4 + ln - 1].decode(), struct.unpack_from("<i", raw, p + 4 + ln)[0]))
        p += 8 + ln
    recs = []
    while p < len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        b = raw[p + 4:p + 4 + bs]
        p += 4 + bs
        ref, pos, l_rn, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, 0)
        name = b[32:32 + l_rn - 1].decode()
        cig = [(w >> 4, OPCH[w & 15]) for w in struct.unpack_from(f"<{n_cig}I", b, 32 + l_rn)]
        a = 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        md = nm = None
        while a + 3 <= len(b):
            tag, ty = b[a:a + 2], chr(b[a + 2])
            a += 3
            if ty in "AcC":
                w = 1
            elif ty in "sS":
                w = 2
            elif ty in "iIf":
                w = 4
            elif ty in "ZH":
                w = b.index(b"\0", a) - a + 1
            elif ty == "B":
                assert tag != b"CG", "the long-CIGAR convention is not part of these fixtures"
                w = 5 + {"c": 1, "C": 1, "s": 2, "S": 2}.get(chr(b[a]), 4) * struct.unpack_from("<i", b, a + 1)[0]
            else:
                raise AssertionError(f"aux type {ty}")
            if tag == b"MD" and ty == "Z":
                md = b[a:a + w - 1]
            if tag == b"NM" and ty in "cCsSiI":
                nm = int.from_bytes(b[a:a + w], "little", signed=ty in "csi")
            a += w
        recs.append(dict(name=name, ref=ref, pos=pos, flag=flag, l_seq=l_seq, cigar=cig, md=md, nm=nm))
    return refs, recs


# ------------------------------------------------------------------ the synthetic cases
REFS = [("chrA", 1000000), ("chrB", 500)]


def _rec(name, cigar, flag=0, l_seq=None, pos=100, ref=0, md=None, nm=None):
    cg = [(int(n), c) for n, c in __import__("re").findall(r"(\d+)([MIDNSHP=X])", cigar)]
    if l_seq is None:
        l_seq = sum(n for n, c in cg if c in "MIS=X")
    return dict(name=name, ref=ref, pos=pos, flag=flag, l_seq=l_seq, cigar=cg, md=md, nm=nm)


def span_cases():
    """every combination of leading H / S / H S and trailing S / H / S H on both strands, the ends the issue lists, MD present / absent / off"""
    out = []
    for li, lead in enumerate(("", "7H", "5S", "7H5S")):
        for ti, trail in enumerate(("", "4S", "9H", "4S9H")):
            for flag in (0, 16):
                out.append(_rec(f"clip_{li}{ti}_{flag}", f"{lead}20=2X3I10=2D8={trail}", flag, pos=100 + 10 * li + ti))
    out += [
        _rec("ends_in_I", "10=3I", 0), _rec("ends_in_ISH", "6H10=3I4S5H", 16), _rec("md_with_eq", "10=2X5M", 0, md=b"17"),
        _rec("md_refines", "14M4D17M", 0, md=b"10A3T0T10^ACGT5"), _rec("md_refines_rev", "3S14M4D17M2H", 16, md=b"10A3T0T10^ACGT5", nm=7),
        _rec("m_without_md", "5S20M3I12M", 16), _rec("m_without_md2", "20M", 0, nm=0), _rec("unmapped", "", 4, l_seq=10, ref=-1, pos=-1),
        _rec("md_long_number", "1234567M", 0, md=b"1234567"), _rec("spliced", "10=500N10=", 0), _rec("pad_first", "3P10=", 0),
        _rec("md_zero_padded", "25M", 0, md=b"0000000000025"),
        _rec("H_behind_the_last_base", "10=5H3S", 0, l_seq=13), _rec("zero_length_ops_behind", "4S10=0D2I0M3S", 16),
        _rec("long_between_ends", "5H" + "3=1X2I4=1D" * 40 + "6=7S", 16),
    ]
    return out


def panic_cases():
    """name -> record whose row is a panic"""
    return {r["name"]: r for r in [
        _rec("ends_in_D", "10=5D"), _rec("ends_in_N", "10=5N"), _rec("starts_with_D", "5D10="), _rec("starts_with_HD", "3H5D10="),
        _rec("H_in_the_middle", "10=3H10="), _rec("H_behind_S", "3S5H10="), _rec("H_between_clips", "5H3P2H10="), _rec("only_I", "10I"), _rec("no_ops", "", l_seq=0), _rec("md_disagrees", "20M", md=b"10A8"),
        _rec("only_S", "10S"), _rec("P_then_D", "2P4D10="),
    ]}


# ------------------------------------------------------------------ MD strings at the kernel's seams
def _md_like(n, seed=1):
    """n bytes that look like an MD value: short numbers, single mismatches, deletions"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        out += b"%d" % int(rng.choice([0, 3, 17, 250, 4096]))
        k = 1 if rng.random() < .7 else int(rng.integers(2, 7))  # one mismatch, or a deletion of up to five bases
        out += (b"" if k == 1 else b"^") + bytes(rng.choice(list(b"ACGT"), k - (k > 1)).astype(np.uint8))
    out = bytes(out[:n])
    return out[:-1] + b"0" if out.endswith(b"^") else out


def _letters(n):
    return (b"ACGT" * (n // 4 + 1))[:n]


def md_cases(shape):
    """-> [(label, string, phase of its first byte (0 .. 15), byte in front of it, byte behind it)] for the shape (bytes per row step, longest
    string a row takes, bytes per wave step) of the kernel under test"""
    row_step, row_max, wave_step = shape
    C = []

    def add(label, s, phase=0, before=b"^", after=b"A"):
        C.append((label, bytes(s), phase, before, after))
    add("KA6", b"10A3T0T10^ACGT")
    add("empty", b"")
    add("999999999", b"999999999")
    add("ten_digits", b"5A1234567890C3")
    add("ten_zeros", b"0000000000A5")
    add("wraps_2^32", b"A".join([b"999999999"] * 5))
    add("caret_digit", b"5^7A")
    add("caret_end", b"12A^")
    add("caret_caret", b"3^^A4")
    add("lower_case", b"5a^c3^Ac")
    add("all_256_bytes", bytes([b for b in range(256) if b != 0x35]) + b"5")  # (the ten digits not in one run)
    add("all_256_bytes_back_and_forth", bytes(range(255, -1, -1)) + bytes(range(256)))
    for phase in range(16):  # hostile neighbours: a digit, a letter, a caret directly in front of the string and at its end
        for before, after in ((b"9", b"9"), (b"^", b"A"), (b"A", b"^"), (b"Z", b"7")):
            nb = (before + after).decode()
            add(f"phase{phase}_{nb}_letters_first", b"ACG12^TT3GA", phase, before, after)
            add(f"phase{phase}_{nb}_digits_first", b"12^AC7T21^AC", phase, before, after)
            add(f"phase{phase}_{nb}_digits_last", b"T120", phase, before, after)
    for n in (1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 5000):
        add(f"deletion_run_{n}", b"7^" + _letters(n) + b"3", phase=n % 16)
        add(f"deletion_run_{n}_to_the_end", b"7^" + _letters(n))
        add(f"letter_run_{n}", b"7" + _letters(n) + b"3", phase=(n + 5) % 16)
        add(f"letter_run_{n}_alone", _letters(n))
    for d in range(1, 10):  # a number of d digits with k of them in front of a lane / step boundary
        num = b"123456789"[:d]
        for k in range(d + 1):
            add(f"lane_split_{d}_{k}", _letters(16 - k) + num + b"C^GT2")
            add(f"row_step_split_{d}_{k}", _md_like(row_step - k - 1) + b"A" + num + b"C^GT2")
            add(f"row_step_split_at_end_{d}_{k}", _md_like(row_step - k - 1) + b"A" + num)
            add(f"wave_step_split_{d}_{k}", _md_like(wave_step - k - 1, 2) + b"A" + num + b"C^GT2" + _md_like(row_max, 3))
            add(f"wave_step_split_at_end_{d}_{k}", _md_like(row_max + wave_step - row_max % wave_step - k - 1, 4) + b"A" + num)
    for label, at, tail in (("lane", 16, b""), ("row_step", row_step, b""), ("wave_step", wave_step, _md_like(row_max, 5))):
        add(f"caret_last_of_{label}", _md_like(at - 2, 6) + b"0^" + b"ACG5" + tail)
        add(f"caret_last_of_{label}_then_digit", _md_like(at - 2, 6) + b"0^" + b"5ACG5" + tail)
        add(f"letters_to_{label}_end", _md_like(at - 5, 7) + b"0^ACG" + b"TTT8" + tail)
    for n in (row_max - 1, row_max, row_max + 1, row_max + 16, 2 * row_max + 3):  # both sides of the row / wave threshold
        add(f"length_{n}", _md_like(n, 8 + n), phase=n % 7)
    return C


def md_layout(cases):
    """-> (text bytes, md_off, md_end): every string at its phase inside a region of carets, digits and letters, its two hostile
    neighbours directly in front of it and behind it; the text ends on a multiple of 16"""
    text, off, end = bytearray(), [], []
    for _, s, phase, before, after in cases:
        text += b"^" * (-len(text) % 16)
        text += (b"9^Z" * 11)[:16 + phase - len(before)] + before
        off.append(len(text))
        text += s
        end.append(len(text))
        text += after
    text += b"^" * (-len(text) % 16)
    return bytes(text), np.array(off, np.uint64), np.array(end, np.uint64)
