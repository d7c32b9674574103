"""Shared by the tests of rb_dev_bam_reads: a plain-Python model of its four outputs on top of bam_rec_util's streams and model (it
knows nothing of the product's code; test_bam_reads_inputs.py holds it to the oracle's nucfreq), a fast twin of model and stream for
files of many uniform records (the scan's seams need a quarter of a million), and the case generators.

A case list is [(label, record body bytes)] as in bam_rec_util; a uniform file is dict(tid, pos, flag, oplen) of numpy columns."""
import struct

import numpy as np

import bam_rec_util as B
import sam_util as U

FILTER = 0x4 | 0x100 | 0x200 | 0x400  # UNMAP | SECONDARY | QCFAIL | DUP: what the pileup never admits
REF_MASK = 0x18D                      # M D N = X
NONE = 2**64 - 1
OUTS = ("seq_off", "start_key", "end_key_pmax")
w = B.w


def nf_key(tid, p):
    """(uint64)(uint32)tid << 32 | min((uint64)p, 0xFFFFFFFF): a negative p saturates"""
    return ((tid & 0xFFFFFFFF) << 32) | min(p & NONE, 0xFFFFFFFF)


def model(data, rec_off, rec_len, m=None):
    """-> dict(seq_off, start_key, end_key_pmax u64 [n], first_unsorted u64 [1], enters bool [n], ref [n] python ints) from the stream and
    bam_rec_util.model's columns"""
    m = B.model(data, rec_off, rec_len) if m is None else m
    n = len(rec_off)
    out = {k: np.zeros(n, np.uint64) for k in OUTS}
    out["enters"], out["ref"] = np.zeros(n, bool), []
    run, first = 0, NONE
    for r in range(n):
        ok = m["status"][r] == B.BAM_OK
        tid, pos, flag = int(m["tid"][r]), int(m["pos"][r]), int(m["flag"][r])
        if ok:
            R = int(rec_off[r])
            out["seq_off"][r] = R + 32 + data[R + 8] + 4 * struct.unpack_from("<H", data, R + 12)[0]  # (the IN-RECORD n_cigar_op)
        ops = m["ops"][int(m["op_off"][r]):int(m["op_off"][r + 1])]
        ref = int((ops[((REF_MASK >> (ops & 15)) & 1) == 1] >> 4).astype(np.uint64).sum()) if len(ops) else 0
        out["ref"].append(ref)
        sk = nf_key(tid, pos)
        out["start_key"][r] = sk
        enters = bool(ok and tid >= 0 and not flag & FILTER)
        out["enters"][r] = enters
        if enters:
            run = max(run, nf_key(tid, max(pos, 0) + (1 if (flag & 4) or ref == 0 else ref)))
        out["end_key_pmax"][r] = run
        if r >= 1 and first == NONE and sk < int(out["start_key"][r - 1]) and tid >= 0 and pos >= 0:
            first = r
    out["first_unsorted"] = np.array([first], np.uint64)
    return out


def slice_of(md, tid, lo_pos, hi_pos):
    """the reads nucfreq_bam hands the device for positions [lo_pos, hi_pos) of tid: [i0, i1), by its two binary searches"""
    k_st, k_en = nf_key(tid, lo_pos), nf_key(tid, hi_pos)
    i0 = int(np.searchsorted(md["end_key_pmax"], np.uint64(k_st), side="right"))
    i1 = i0 + int(np.searchsorted(md["start_key"][i0:], np.uint64(k_en), side="left"))
    return i0, max(i0, i1)


# ------------------------------------------------------------------ uniform files: one op, name "r", no SEQ, no aux
UNIFORM_DT = np.dtype([("bs", "<u4"), ("tid", "<i4"), ("pos", "<i4"), ("l_rn", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cig", "<u2"), ("flag", "<u2"),
                       ("l_seq", "<u4"), ("next", "<i4", 3), ("name", "S2"), ("op", "<u4")])


def uniform_stream(u):
    """-> (data, rec_off, rec_len) of the records (tid, pos, flag, one op of length oplen[i] and nibble opc[i] (default M))"""
    n = len(u["tid"])
    rec = np.zeros(n, UNIFORM_DT)
    rec["bs"], rec["tid"], rec["pos"], rec["flag"] = UNIFORM_DT.itemsize - 4, u["tid"], u["pos"], u["flag"]
    rec["l_rn"], rec["mapq"], rec["n_cig"], rec["name"] = 2, 60, 1, b"r"
    rec["next"] = (-1, -1, 0)
    rec["op"] = (np.asarray(u["oplen"], np.uint32) << 4) | np.asarray(u.get("opc", 0), np.uint32)
    head = U.bam_bytes(B.REFS, [])
    off = len(head) + 4 + UNIFORM_DT.itemsize * np.arange(n, dtype=np.uint64)
    return head + rec.tobytes(), off, np.full(n, UNIFORM_DT.itemsize - 4, np.uint32)


def uniform_model(u, rec_off):
    """what bam_rec_util.model and model() give for uniform_stream(u), in numpy (test_bam_reads_inputs.py compares them)"""
    n = len(u["tid"])
    tid, pos, flag = np.asarray(u["tid"], np.int64), np.asarray(u["pos"], np.int64), np.asarray(u["flag"], np.int64)
    oplen, opc = np.asarray(u["oplen"], np.int64), np.broadcast_to(np.asarray(u.get("opc", 0), np.int64), (n,))
    mapped = (flag & 4) == 0
    c = dict(tid=tid.astype(np.int32), pos=pos, flag=flag.astype(np.uint32), l_seq=np.zeros(n, np.uint32), has_md=np.zeros(n, np.uint8),
             md_off=np.zeros(n, np.uint64), md_end=np.zeros(n, np.uint64), status=np.zeros(n, np.uint8))
    c["op_off"] = np.concatenate([[0], np.cumsum(mapped)]).astype(np.uint64)
    c["ops"] = ((oplen << 4) | opc)[mapped].astype(np.uint32)
    ref = np.where(mapped & (((REF_MASK >> opc) & 1) == 1), oplen, 0)
    key = lambda t, p: ((t & 0xFFFFFFFF).astype(np.uint64) << np.uint64(32)) | np.where(p < 0, 0xFFFFFFFF, np.minimum(p, 0xFFFFFFFF)).astype(np.uint64)
    sk = key(tid, pos)
    enters = (tid >= 0) & ((flag & FILTER) == 0)
    ek = np.where(enters, key(tid, np.maximum(pos, 0) + np.where(ref == 0, 1, ref)), 0).astype(np.uint64)
    cand = np.flatnonzero((sk[1:] < sk[:-1]) & (tid[1:] >= 0) & (pos[1:] >= 0)) + 1
    c.update(seq_off=np.asarray(rec_off, np.uint64) + np.uint64(32 + 2 + 4), start_key=sk,
             end_key_pmax=np.maximum.accumulate(ek) if n else ek, first_unsorted=np.array([cand[0] if len(cand) else NONE], np.uint64), enters=enters)
    return c


def scan_file(n, blk):
    """n sorted records on three contigs whose end keys put the scan's carries to work: in every even workgroup of `blk` records the
    largest end lies in its FIRST record, in every odd one in its LAST; runs of reads that do not enter lie across the first seams; the
    contig steps at n / 3 and 2 n / 3"""
    i = np.arange(n, dtype=np.int64)
    tid = (3 * i) // max(n, 1)
    pos = 7 * (i - np.searchsorted(tid, tid, side="left")) + 5
    oplen = np.full(n, 11, np.int64)
    b, j = i // blk, i % blk
    oplen[(b % 2 == 0) & (j == 0)] = 7 * blk + 100000   # reaches behind everything in its workgroup
    oplen[(b % 2 == 1) & (j == blk - 1)] = 300000
    flag = np.where(i % 5 == 3, 16, 0)
    flag[(i % 97 == 50) & (j != 0) & (j != blk - 1)] = 0x100
    for seam, half in ((blk, 9), (3 * blk, 2), (blk * blk, 3)):
        flag[(i >= seam - half) & (i < seam + half)] = 0x400
    return dict(tid=tid, pos=pos, flag=flag, oplen=oplen)


def scan_counts(blk):
    """the record counts of the issue: 0, 1, a wavefront's seams, a workgroup's, and enough workgroups to reach the scan's top level, plus 1"""
    return [0, 1, 63, 64, 65, blk - 1, blk, blk + 1, blk * blk, blk * blk + 1]


def unsorted_files(n=300):
    """label -> (uniform file, first_unsorted)"""
    def base():
        i = np.arange(n, dtype=np.int64)
        return dict(tid=np.zeros(n, np.int64), pos=10 * i + 10, flag=np.zeros(n, np.int64), oplen=np.full(n, 5, np.int64))
    out = {"none": (base(), NONE)}
    u = base()
    u["pos"][1] = 3
    out["at_1"] = (u, 1)
    u = base()
    u["pos"][n - 1] = 3
    out["at_n-1"] = (u, n - 1)
    u = base()
    u["pos"][70], u["pos"][200] = 3, 3   # (records 70 and 200: different wavefronts, different workgroups; 71 and 201 are not candidates: they lie behind 69 / 199 only by value)
    out["two_candidates_the_smaller_wins"] = (u, 70)
    u = base()
    u["pos"][200], u["pos"][71] = 3, 3
    out["two_candidates_written_in_the_other_order"] = (u, 71)
    u = base()
    u["tid"][n - 2:], u["pos"][n - 2], u["pos"][n - 1] = -1, 100, 50  # (tid < 0: behind one another, and no candidate)
    out["masked_by_tid"] = (u, NONE)
    u = base()
    u["tid"][100:], u["tid"][150], u["pos"][150] = 1, 0, -1            # (key (0, 2^32 - 1) behind (1, ..): pos < 0 is no candidate)
    out["masked_by_pos"] = (u, NONE)
    return out


# ------------------------------------------------------------------ the cases (general records)
def seq_cases():
    """SEQ at every byte phase: l_read_name 1 .. 17 x n_cigar 0 .. 3; l_seq 0 and odd; a CG:B,I record of 70000 words behind two in-record
    words; every refusal"""
    C = []
    for l_rn in range(1, 18):
        for nc in range(4):
            C.append((f"seq_{l_rn}_{nc}", B.body(name=b"n" * (l_rn - 1) + b"\0", pos=100 + l_rn, words=[w(3 + k, "M") for k in range(nc)], l_seq=(l_rn * 3 + nc) % 7)))
    C.append(("l_seq_0", B.body(name=b"z\0", pos=200, words=[w(9, "=")], l_seq=0)))
    C.append(("l_seq_odd", B.body(name=b"z\0", pos=201, words=[w(9, "=")], l_seq=9)))
    C.append(("cg_70000", B.body(name=b"cg\0", pos=300, words=[w(5, "S"), w(100, "N")], l_seq=5, aux=B.scalar("i") + B.cg(B._words(70000, 7)))))
    return C + B.status_cases()


def ref_cases(shape):
    """the reference sum: op counts at every seam of the row and wavefront form, ops that consume no reference, a sum behind 2^32, every nibble"""
    counts = sorted({0, 1, 15, 16, 17} | {v + d for v in shape for d in (-1, 0, 1)})
    C, cum = [], 0
    for k, nc in enumerate(counts):
        for lead in range(4):  # (a filler in front turns the CIGAR's first op to dword `lead` of its 16-byte group)
            f = (lead - cum) % 4
            C.append((f"filler_{nc}_{lead}", B.body(name=b"f\0", pos=10 * k, words=B._words(f, k))))
            C.append((f"ops_{nc}_{lead}", B.body(name=b"o\0", pos=10 * k + 1 + lead, words=B._words(nc, 31 * nc + lead))))
            cum += f + nc
    C.append(("only_I_S_H_P", B.body(name=b"q\0", pos=5000, words=[w(3, "H"), w(4, "S"), w(5, "I"), w(6, "P"), w(7, "S")], l_seq=16)))
    C.append(("sum_behind_2^32", B.body(name=b"q\0", pos=5001, words=[w(2**28 - 1, "D" if k % 2 else "M") for k in range(20)], l_seq=4)))
    C.append(("sum_behind_2^32_negative_pos", B.body(name=b"q\0", pos=-5, words=[w(2**28 - 1, "N") for _ in range(20)])))
    C.append(("every_nibble", B.body(name=b"q\0", pos=5002, words=[((k + 2) << 4) | k for k in range(16)])))
    C.append(("endpos_2^32", B.body(name=b"q\0", pos=2**31 - 1, words=[w(2**28 - 1, "M")] * 8 + [w(9, "M")])))    # (saturates by one)
    C.append(("endpos_2^32-1", B.body(name=b"q\0", pos=2**31 - 1, words=[w(2**28 - 1, "M")] * 8 + [w(8, "M")])))  # (0xFFFFFFFF without saturating)
    return C


def enters_cases():
    C = []
    long_read = dict(words=[w(100000, "M")])
    for bit in (0x4, 0x100, 0x200, 0x400):
        C.append((f"flag_{bit:#x}_alone", B.body(name=b"e\0", pos=100, flag=bit, **long_read)))
        C.append((f"behind_flag_{bit:#x}", B.body(name=b"e\0", pos=101, words=[w(3, "M")])))
    for bit in (0x1, 0x2, 0x8, 0x10, 0x20, 0x40, 0x80, 0x800):
        C.append((f"flag_{bit:#x}_enters", B.body(name=b"e\0", pos=102, flag=bit, words=[w(200000 + bit, "M")])))
    C.append(("tid_-1", B.body(name=b"e\0", tid=-1, pos=103, **long_read)))
    C.append(("pos_-1_tid_0", B.body(name=b"e\0", tid=0, pos=-1, words=[w(300000, "M")])))
    C.append(("refused", B.body(name=b"e", pos=104, **long_read)))  # (no NUL behind the name)
    C.append(("unmapped_with_a_cigar", B.body(name=b"e\0", tid=1, pos=105, flag=4, **long_read)))
    C.append(("unmapped_placed_enters_nothing", B.body(name=b"e\0", tid=1, pos=2**30, flag=4)))
    C.append(("no_ops_reaches_pos_plus_1", B.body(name=b"e\0", tid=1, pos=2**30 + 5)))
    C.append(("tid_step", B.body(name=b"e\0", tid=1, pos=3, words=[w(3, "M")])))
    return C


# ------------------------------------------------------------------ records with bases (the composition with nucfreq)
def body_with_seq(name, tid, pos, flag, words, nibbles):
    """bam_rec_util.body with the read's bases in place of its 0xFF"""
    l_seq = len(nibbles)
    b = bytearray(B.body(name=name, tid=tid, pos=pos, flag=flag, words=words, l_seq=l_seq))
    s = list(nibbles) + [0]
    at = 32 + len(name) + 4 * len(words)
    b[at:at + (l_seq + 1) // 2] = bytes((s[k] << 4) | s[k + 1] for k in range(0, l_seq, 2))
    return bytes(b)


def reads_stream(reads):
    """an nf_util.Reads set as a BAM stream: names of every length 1 .. 16 move SEQ through the byte phases; one unmapped record of 64
    bases closes the file (32 readable bytes behind the last read's SEQ)"""
    bodies = []
    for i in range(reads.n):
        ops = reads.ops[int(reads.op_off[i]):int(reads.op_off[i + 1])]
        a = int(reads.seq_off[i])
        ls = int(reads.l_seq[i])
        nib = [int(x) for byte in reads.seq[a:a + (ls + 1) // 2] for x in (byte >> 4, byte & 15)][:ls]
        bodies.append(body_with_seq(b"n" * (i % 16) + b"\0", int(reads.tid[i]), int(reads.pos[i]), int(reads.flag[i]), ops, nib))
    bodies.append(B.body(name=b"end\0", tid=-1, pos=-1, flag=4, l_seq=64))
    return B.stream(bodies)


# ------------------------------------------------------------------ a BGZF file with a .bai of its own (the index ranges of rb nucfreq)
def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def bgzf_and_bai(refs, recs, member=512, cut_in=None):
    """sam_util records (sorted; unmapped ones last) -> (BGZF bytes in members of `member` uncompressed bytes, .bai bytes, record starts in
    the stream).  cut_in = r: the index ends INSIDE record r -- its chunk stops 10 bytes into the record and the later records of its bin
    are left out --, so a reader that trusts the index finds the record cut off where the chunk's last member ends"""
    data = U.bam_bytes(refs, recs)
    raw = U.bgzf_bytes(data, (member,))
    coff, at = [], 0
    while at < len(raw):
        coff.append(at)
        at += struct.unpack_from("<H", raw, at + 16)[0] + 1
    voff = lambda u: (coff[u // member] << 16) | (u % member)  # noqa: E731
    _, off, ln = B.hop(data)
    start = [int(o) - 4 for o in off]
    per = [dict(bins={}, lin={}) for _ in refs]
    cut_bin = None
    for r, rec in enumerate(recs):
        if rec["ref"] < 0:
            continue
        b, e = rec["pos"], rec["pos"] + max(sum(k for k, c in rec["cigar"] if c in "MDN=X"), 1)
        key = (rec["ref"], reg2bin(b, e))
        if key == cut_bin:
            continue
        v0, v1 = voff(start[r]), voff(start[r] + 4 + int(ln[r]))
        if r == cut_in:
            v1, cut_bin = voff(start[r] + 10), key
        ch = per[rec["ref"]]["bins"].setdefault(key[1], [])
        if ch and ch[-1][1] == v0:
            ch[-1][1] = v1
        else:
            ch.append([v0, v1])
        lin = per[rec["ref"]]["lin"]
        for x in range(b >> 14, ((e - 1) >> 14) + 1):
            lin[x] = min(lin.get(x, v0), v0)
    bai = b"BAI\x01" + struct.pack("<i", len(refs))
    for p in per:
        bai += struct.pack("<i", len(p["bins"]))
        for k, ch in p["bins"].items():
            bai += struct.pack("<Ii", k, len(ch)) + b"".join(struct.pack("<QQ", x, y) for x, y in ch)
        n_intv = max(p["lin"]) + 1 if p["lin"] else 0
        io = [p["lin"].get(x, 0) for x in range(n_intv)]
        for x in range(n_intv - 2, -1, -1):  # windows nobody overlaps take the next window's offset, as samtools writes them
            if io[x] == 0:
                io[x] = io[x + 1]
        bai += struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", x) for x in io)
    return raw, bai, start


def three_islands():
    """-> (refs, recs, beds): three groups of 30 reads far apart in the file (fillers of dozens of BGZF members between them), and a BED of
    one small region per group, contigs interleaved: the index gives three disjoint ranges of members"""
    refs = [("chrA", 50000), ("chrB", 30000)]
    mk = lambda nm, ref, pos, i: dict(name=f"{nm}{i:03d}", ref=ref, pos=pos, flag=16 if i % 3 == 0 else 0, l_seq=40, cigar=[(3, "S"), (30, "M"), (2, "D"), (7, "M")])  # noqa: E731
    recs = [mk("a", 0, 100 + 3 * i, i) for i in range(30)] + [mk("f", 0, 20000 + 5 * i, i) for i in range(150)] + [mk("b", 0, 40000 + 3 * i, i) for i in range(30)]
    recs += [mk("g", 1, 100 + 5 * i, i) for i in range(100)] + [mk("c", 1, 20000 + 3 * i, i) for i in range(30)]
    recs.append(dict(name="un", ref=-1, pos=-1, flag=4, l_seq=5, cigar=[]))
    bed = "chrB\t20000\t20300\tthird\nchrA\t100\t400\tfirst\nchrA\t40000\t40300\nchrA\t150\t160\n"
    return refs, recs, bed
