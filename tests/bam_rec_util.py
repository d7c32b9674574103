"""Shared by the tests of rb_dev_bam_records: BAM records built byte by byte on top of sam_util.bam_bytes (arbitrary aux lists, CG tags,
hand-set l_read_name / n_cigar / l_seq / block_size), the hop from record to record, and a plain-Python model of the call's rules that
knows nothing of the product's code (test_bam_rec_inputs.py holds it to sam_util.read_bam and to the oracle).

A stream is (data bytes, rec_off u64 [n], rec_len u32 [n]); a case list is [(label, record body bytes)]."""
import struct

import numpy as np

import sam_util as U

BAM_OK, BAM_SHORT_BLOCK, BAM_NO_FIT, BAM_BAD_NAME = 0, 1, 2, 3
REFS = U.REFS
COLS = ("tid", "pos", "flag", "l_seq", "has_md", "md_off", "md_end", "status")
OP = {c: i for i, c in enumerate(U.OPCH)}
INT32_MIN = -2**31
MD20 = b"10A5^AC4"  # an MD that accounts for 20 bases of M


def w(ln, op):
    return (ln << 4) | OP[op]


# ------------------------------------------------------------------ records
def body(name=b"r\0", tid=0, pos=100, flag=0, words=(), l_seq=0, aux=b"", l_read_name=None, n_cigar=None, l_seq_field=None, cut=None):
    """one record without its block_size field.  name: the bytes of the name field as they are (NUL included, or not); words: the
    in-record CIGAR words; l_read_name / n_cigar / l_seq_field: what the fixed fields SAY (default: what is there); cut: keep only
    that many bytes"""
    words = np.asarray(words, np.uint32)
    b = struct.pack("<iiBBHHHIiii", tid, pos, len(name) if l_read_name is None else l_read_name, 60, 0, len(words) if n_cigar is None else n_cigar,
                    flag, l_seq if l_seq_field is None else l_seq_field, -1, -1, 0)
    b += bytes(name) + words.astype("<u4").tobytes() + b"\xff" * ((l_seq + 1) // 2) + b"\xff" * l_seq + bytes(aux)
    return b if cut is None else b[:cut]


def stream(bodies, refs=REFS):
    """-> (data, rec_off, rec_len): the header of sam_util.bam_bytes, then every body behind its block_size"""
    out = bytearray(U.bam_bytes(refs, []))
    off, ln = [], []
    for b in bodies:
        out += struct.pack("<I", len(b))
        off.append(len(out))
        ln.append(len(b))
        out += b
    return bytes(out), np.array(off, np.uint64), np.array(ln, np.uint32)


def hop(data):
    """-> (refs, rec_off, rec_len) of an uncompressed BAM stream: the host's part of the decode"""
    assert data[:4] == b"BAM\x01"
    p = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, p)[0]
    p += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", data, p)[0]
        refs.append((data[p + 4:p + 4 + ln - 1].decode(), struct.unpack_from("<i", data, p + 4 + ln)[0]))
        p += 8 + ln
    off, ln = [], []
    while p < len(data):
        bs = struct.unpack_from("<I", data, p)[0]
        assert p + 4 + bs <= len(data)
        off.append(p + 4)
        ln.append(bs)
        p += 4 + bs
    return refs, np.array(off, np.uint64), np.array(ln, np.uint32)


# ------------------------------------------------------------------ aux fields
SCALARS = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
B_SUB = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def scalar(ty, tag=b"XX", fill=0x41):
    return tag + ty.encode() + bytes([fill]) * SCALARS[ty]


def z(tag, s, ty="Z", nul=True):
    return tag + ty.encode() + bytes(s) + (b"\0" if nul else b"")


def md(s, nul=True):
    return z(b"MD", s, nul=nul)


def barr(tag, sub, count, payload=None, say=None):
    """a B array of `count` elements (payload: their bytes, default 0x42 ...); say: the count the head states"""
    payload = bytes([0x42]) * (B_SUB.get(sub, 4) * count) if payload is None else bytes(payload)
    return tag + b"B" + sub.encode() + struct.pack("<I", count if say is None else say) + payload


def cg(words, sub="I"):
    words = np.asarray(words, "<u4")
    return barr(b"CG", sub, len(words), words.tobytes())


# ------------------------------------------------------------------ the model
def model(data, rec_off, rec_len):
    """-> dict(tid i32, pos i64, flag u32, l_seq u32, has_md u8, md_off u64, md_end u64, status u8 [n], op_off u64 [n + 1], ops u32)"""
    n = len(rec_off)
    c = dict(tid=np.zeros(n, np.int32), pos=np.zeros(n, np.int64), flag=np.zeros(n, np.uint32), l_seq=np.zeros(n, np.uint32), has_md=np.zeros(n, np.uint8),
             md_off=np.zeros(n, np.uint64), md_end=np.zeros(n, np.uint64), status=np.zeros(n, np.uint8), op_off=np.zeros(n + 1, np.uint64))
    ops = []
    for r in range(n):
        R, bs = int(rec_off[r]), int(rec_len[r])
        b = data[R:R + bs]
        assert len(b) == bs
        c["op_off"][r + 1] = c["op_off"][r]
        if bs < 32:
            c["status"][r] = BAM_SHORT_BLOCK
            continue
        tid, pos, l_rn, _mq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", b, 0)
        need = 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        if need > bs:
            c["status"][r] = BAM_NO_FIT
            continue
        if l_rn == 0 or b[32 + l_rn - 1] != 0:
            c["status"][r] = BAM_BAD_NAME
            continue
        c["tid"][r], c["pos"][r], c["flag"][r], c["l_seq"][r] = tid, pos, flag, l_seq
        if flag & 4:
            continue
        p, md_at, cg_at = need, None, None
        while p + 3 <= bs:
            tag, ty = b[p:p + 2], chr(b[p + 2])
            p += 3
            if ty in SCALARS:
                p += SCALARS[ty]
            elif ty in "ZH":
                q = b.find(b"\0", p)
                q = bs if q < 0 else q
                if tag == b"MD" and ty == "Z":
                    md_at = (p, q)
                p = q + 1
            elif ty == "B":
                if p + 5 > bs:
                    break
                sub, cnt = chr(b[p]), struct.unpack_from("<I", b, p + 1)[0]
                es = B_SUB.get(sub, 4)
                if p + 5 + es * cnt > bs:
                    break
                if tag == b"CG" and sub == "I":
                    cg_at = (p + 5, cnt)
                p += 5 + es * cnt
            else:
                break
        if md_at is not None:
            c["has_md"][r], c["md_off"][r], c["md_end"][r] = 1, R + md_at[0], R + md_at[1]
        at, cnt = 32 + l_rn, n_cig
        if cg_at is not None and n_cig >= 1:
            first = struct.unpack_from("<I", b, at)[0]
            if first & 15 == 4 and first >> 4 == l_seq:
                at, cnt = cg_at
        ops.append(np.frombuffer(b, "<u4", cnt, at) if cnt else np.zeros(0, np.uint32))
        c["op_off"][r + 1] += cnt
    c["ops"] = np.concatenate(ops + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return c


def source_of(data, rec_off, rec_len, m):
    """-> per record the byte in data where its ops lie (None: no ops): the in-record words, or the CG tag's"""
    out = []
    for r in range(len(rec_off)):
        cnt = int(m["op_off"][r + 1] - m["op_off"][r])
        if not cnt:
            out.append(None)
            continue
        R, b = int(rec_off[r]), data[int(rec_off[r]):int(rec_off[r]) + int(rec_len[r])]
        l_rn, n_cig = b[8], struct.unpack_from("<H", b, 12)[0]
        at = R + 32 + l_rn
        if not (cnt == n_cig and data[at:at + 4 * cnt] == m["ops"][int(m["op_off"][r]):int(m["op_off"][r + 1])].astype("<u4").tobytes()):
            at = R + b.index(b"CGBI" + struct.pack("<I", cnt)) + 8  # (the case generators put one such tag in a record)
        out.append(at)
    return out


def records_of(data, rec_off, rec_len, m, refs):
    """the model's columns as sam_util records (what read_bam returns, nm apart)"""
    recs = []
    for r in range(len(rec_off)):
        assert m["status"][r] == BAM_OK
        R = int(rec_off[r])
        l_rn = data[R + 8]
        name = data[R + 32:R + 32 + l_rn - 1].decode()
        words = m["ops"][int(m["op_off"][r]):int(m["op_off"][r + 1])]
        mdv = data[int(m["md_off"][r]):int(m["md_end"][r])] if m["has_md"][r] else None
        recs.append(dict(name=name, ref=int(m["tid"][r]), pos=int(m["pos"][r]), flag=int(m["flag"][r]), l_seq=int(m["l_seq"][r]),
                         cigar=[(int(x) >> 4, U.OPCH[int(x) & 15]) for x in words], md=mdv, nm=None))
    return recs


# ------------------------------------------------------------------ the cases
N_CIGARS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65)


def _words(n, seed):
    """n words of a plausible CIGAR whose content differs from word to word (a misplaced word shows)"""
    k = np.arange(n, dtype=np.uint32)
    out = ((((k * np.uint32(2654435761) + np.uint32(seed)) >> np.uint32(8)) & np.uint32(0xFF0)) | np.uint32(0x10) | (np.array([0, 1, 0, 2, 7, 8, 0, 3], np.uint32)[k % 8])).astype(np.uint32)
    if n:
        out[-1] &= np.uint32(0xFFFFFFF0)  # (the last op an M: the reference's read_pos wants the span to end in one)
    return out


def gather_cases(copy_row_max):
    """l_read_name 1 .. 20 x every n_cigar of the issue's list (and one below, at, above the copy's row / wave threshold), each four times
    behind a filler record whose op count turns the destination to the next dword phase"""
    out, cum, at, c = [], 0, len(U.bam_bytes(REFS, [])), 0
    for nc in N_CIGARS + (copy_row_max - 1, copy_row_max, copy_row_max + 1):
        for l_rn in range(1, 21):
            for d in range(4):
                f = (d - cum) % 4
                # the filler's name is as long as puts the record's words at byte (c + 5 d) mod 16 of a group (in a stream of stream())
                fn = 1 + (c + 5 * d - (at + 72 + 4 * f + l_rn) - 1) % 16
                out.append((f"filler_{nc}_{l_rn}_{d}", body(name=b"f" * (fn - 1) + b"\0", words=_words(f, 1))))
                out.append((f"gather_{nc}_{l_rn}_{d}", body(name=b"n" * (l_rn - 1) + b"\0", words=_words(nc, 100 * l_rn + d))))
                cum += f + nc
                at += 8 + len(out[-2][1]) + len(out[-1][1])
            c += 1
    return out


def aux_cases(aux_row_max):
    C = []
    m10 = MD20

    def add(label, aux, mdv=MD20, **kw):
        """mdv: the MD the record ends up with; its CIGAR is one M of as many bases as that MD accounts for (the reference asserts it)"""
        k = sum(U.md_host(mdv)[:2])
        kw.setdefault("words", [w(k, "M")] if 0 < k < 2**28 else [w(20, "=")])
        kw.setdefault("l_seq", 20)
        C.append((label, body(name=label.encode()[:40] + b"\0", aux=aux, **kw)))
    front = b"".join(scalar(t, b"X" + t.encode()) for t in SCALARS) + b"".join(barr(b"Y" + s.encode(), s, 3) for s in B_SUB)
    add("every_type_in_front", front + md(m10))
    for t in SCALARS:
        add(f"scalar_{t}_in_front", scalar(t) + md(m10))
    for s in B_SUB:
        for cnt in (0, 1, 5):
            add(f"B{s}_{cnt}_in_front", barr(b"YY", s, cnt) + md(m10))
    add("B_unknown_subtype_counts_4", barr(b"YY", "d", 2, bytes(8)) + md(m10))
    add("md_first", md(m10) + scalar("i") + z(b"RG", b"grp1"))
    add("md_middle", scalar("i") + md(m10) + z(b"RG", b"grp1"))
    add("md_last", scalar("i") + z(b"RG", b"grp1") + md(m10))
    add("md_absent", scalar("i") + z(b"RG", b"grp1"))
    add("no_aux", b"")
    add("md_twice", md(b"7A7") + scalar("C") + md(m10))
    add("md_twice_second_empty", md(m10) + md(b""), mdv=b"")
    add("md_as_H_is_not_md", z(b"MD", b"1A2B", ty="H") + scalar("c"))
    add("md_as_i_is_not_md", scalar("i", b"MD"))
    add("H_in_front", z(b"HX", b"00FF", ty="H") + md(m10))
    add("Z_with_md_inside", z(b"CO", b"MDZ9A9") + md(m10))
    for n in list(range(34)) + [255, 256, 257, 5000]:
        s = U._md_like(n, 3 + n) if n else b""
        add(f"md_len_{n}", scalar("s") * (n % 3) + md(s), mdv=s)
    for phase in range(16):  # the NUL at every byte of a 16-byte group: the name's length moves everything
        pad = (12 - (32 + phase + 1 + 4 + 5 + 9 + 7 + 4)) % 16  # (record and block_size field: a multiple of 16, so that only the name moves the NUL)
        C.append((f"nul_phase_{phase}", body(name=b"p" * phase + b"\0", words=[w(9, "M")], l_seq=9, aux=md(b"4C4") + z(b"XX", b"x" * pad))))
    fixed = len(scalar("i")) + 3 + 1  # an i field, the MD's head and NUL
    for d in (-1, 0, 1):  # the aux area one below, at, above the row / wave threshold; then the same with the MD in front
        n = aux_row_max + d - fixed
        add(f"aux_area_{aux_row_max + d}", scalar("i") + md(U._md_like(n, 7)), mdv=U._md_like(n, 7))
        add(f"aux_area_{aux_row_max + d}_md_first", md(U._md_like(n, 8)) + scalar("i"), mdv=U._md_like(n, 8))
    big = aux_row_max + 1000  # (the wavefront form, whatever the threshold)
    add("wave_many_small_fields", scalar("C") * (big // 4) + md(m10) + scalar("s") * 3)
    add("wave_long_Z_then_md", z(b"CO", b"x" * big) + md(m10) + barr(b"YY", "S", 4))
    add("wave_md_unterminated", scalar("i") * (big // 7) + md(U._md_like(700, 9), nul=False))
    add("wave_two_mds", md(U._md_like(big, 10)) + md(U._md_like(2500, 11)), mdv=U._md_like(2500, 11))
    add("md_unterminated", scalar("i") + md(b"3A3", nul=False))
    add("md_unterminated_empty", scalar("i") + md(b"", nul=False))
    add("Z_unterminated_behind_md", md(m10) + z(b"CO", b"no end", nul=False))
    add("unknown_type_in_front", b"XXq\1\2\3\4" + md(m10))
    add("unknown_type_behind", md(m10) + b"XXq\1\2\3\4" + md(b"9"))
    add("B_head_overruns", md(m10) + b"YYBI\2\0")
    add("B_head_overruns_by_one", md(m10) + b"YYBI\2\0\0")
    add("B_array_overruns", md(m10) + barr(b"YY", "I", 2, say=3))
    add("B_array_overruns_2^32", md(m10) + barr(b"YY", "I", 2, say=0xFFFFFFFF) + md(b"9"))
    add("B_array_overrun_hides_md", barr(b"YY", "s", 2, say=40) + md(b"9"))
    add("B_array_fits_exactly", md(m10) + barr(b"YY", "s", 7))
    for k in range(4):
        add(f"left_behind_{k}", md(m10) + scalar("i") + b"ZZ\0"[:k])
    add("left_behind_3_is_a_head", md(m10) + b"XXC")  # (a head whose value lies behind the record: the walk steps past the end)
    return C


def cg_cases():
    C = []
    L = 5

    def add(label, words, aux, l_seq=L, name=None, **kw):
        C.append((label, body(name=(name or label.encode()[:40]) + b"\0", words=words, l_seq=l_seq, aux=aux, **kw)))
    real3 = [w(2, "S"), w(3, "M"), w(4, "I")]
    conv = [w(L, "S"), w(100, "N")]
    add("applies_3", conv, cg(real3))
    for n in (65536, 70000):
        add(f"applies_{n}", conv, scalar("i") + cg(_words(n, n)) + z(b"RG", b"g"))
    add("applies_one_word_in_record", [w(L, "S")], cg(real3))
    add("applies_zero_words_in_tag", conv, cg([]))
    add("first_op_not_S", [w(L, "M"), w(100, "N")], cg(real3))
    add("S_length_is_not_l_seq", [w(L + 1, "S"), w(100, "N")], cg(real3))
    add("n_cigar_0", [], cg(real3))
    add("subtype_i", conv, cg(real3, "i"))
    add("subtype_S", conv, barr(b"CG", "S", 6, np.asarray(real3, "<u4").tobytes()))
    add("tag_is_not_CG", conv, barr(b"CH", "I", 3, np.asarray(real3, "<u4").tobytes()))
    add("two_tags_the_last_wins", conv, cg(real3[:2]) + cg(real3))
    add("in_front_of_md", conv, cg(real3) + md(b"3"))
    add("behind_md", conv, md(b"3") + cg(real3))
    add("overrunning_tag_is_not_seen", conv, md(b"3") + barr(b"CG", "I", 3, np.asarray(real3, "<u4").tobytes(), say=4))
    add("unmapped_with_tag", conv, cg(real3), flag=4)
    for phase in range(16):
        pad = (12 - (32 + phase + 1 + 8 + 3 + 5 + 4 + 8 + 84 + 4)) % 16  # (record and block_size field: a multiple of 16, so that only the name moves the tag)
        add(f"tag_phase_{phase}", conv, scalar("C") + cg(_words(21, phase)) + z(b"XX", b"x" * pad), name=b"q" * phase)
    return C


def status_cases():
    C = []
    ok = body(name=b"ok\0", words=[w(7, "M")], l_seq=7, aux=md(b"7"))
    C.append(("block_size_31", body(name=b"\0", cut=31)))
    C.append(("block_size_0", b""))
    C.append(("block_size_32_no_name", body(name=b"", l_read_name=0)))
    C.append(("block_size_32_says_a_name", body(name=b"", l_read_name=1)))
    C.append(("block_size_33", body(name=b"\0")))
    C.append(("fits_exactly", body(name=b"ab\0", words=[w(3, "M")], l_seq=3)))
    C.append(("short_by_one", body(name=b"ab\0", words=[w(3, "M")], l_seq=3, cut=32 + 3 + 4 + 2 + 3 - 1)))
    C.append(("l_seq_2^32-1", body(name=b"ab\0", words=[w(3, "M")], l_seq=3, l_seq_field=0xFFFFFFFF)))
    C.append(("l_seq_2^32-2", body(name=b"ab\0", words=[w(3, "M")], l_seq=3, l_seq_field=0xFFFFFFFE)))
    C.append(("l_seq_wraps_to_fit_in_32_bits", body(name=b"ab\0", words=[], l_seq=0, l_seq_field=0xAAAAAAAA, aux=scalar("i") * 4)))  # 3/2 x + .. = 2^32 + small
    C.append(("n_cigar_says_more", body(name=b"ab\0", words=[w(3, "M")], l_seq=3, n_cigar=0xFFFF)))
    C.append(("l_read_name_0", body(name=b"", l_read_name=0, words=[w(3, "M")], l_seq=3, aux=md(b"3"))))
    C.append(("name_without_nul", body(name=b"abc", words=[w(3, "M")], l_seq=3, aux=md(b"3"))))
    C.append(("name_nul_only_inside", body(name=b"a\0c", words=[w(3, "M")], l_seq=3)))
    C.append(("name_255", body(name=b"n" * 254 + b"\0", words=[w(3, "M")], l_seq=3, aux=md(b"3"))))
    C.append(("no_fit_comes_before_bad_name", body(name=b"abc", l_read_name=0, words=[w(3, "M")], l_seq=3, l_seq_field=1000)))
    C.append(("short_block_comes_first", body(name=b"", l_read_name=0, l_seq_field=0xFFFFFFFF, cut=20)))
    C.append(("broken_unmapped_no_fit", body(name=b"u\0", flag=4, l_seq=4, cut=36)))
    C.append(("broken_unmapped_bad_name", body(name=b"u", flag=4, l_seq=4)))
    C.append(("good_unmapped", body(name=b"u\0", flag=4, tid=-1, pos=-1, l_seq=4, words=[w(4, "M")], aux=md(b"4"))))
    return [("ok_in_front", ok)] + C + [("ok_behind", ok)]


def field_cases():
    C = []
    for tid in (-1, INT32_MIN, 2**31 - 1):
        for pos in (-1, INT32_MIN, 2**31 - 1):
            C.append((f"tid_{tid}_pos_{pos}", body(name=b"t\0", tid=tid, pos=pos, words=[w(3, "=")], l_seq=3)))
    C.append(("flag_FFFF", body(name=b"t\0", flag=0xFFFF, words=[w(3, "=")], l_seq=3)))
    C.append(("flag_FFFB", body(name=b"t\0", flag=0xFFFB, words=[w(3, "=")], l_seq=3, aux=md(b"3"))))
    C.append(("l_seq_0", body(name=b"t\0", words=[w(3, "=")], l_seq=0, aux=md(b"3"))))
    C.append(("op_nibbles_9_to_15", body(name=b"t\0", words=[(5 << 4) | k for k in range(9, 16)], l_seq=0)))
    return C
