"""Inputs and bindings for the liftover --qbed tests: the record sets rb_dev_swap is run in place on (tests/test_gpu_swap_inplace.py), the
batch and windows of the RB_LIFT_QBED wrapper test (tests/test_gpu_qbed_text.py), ctypes bindings of the text wrappers -- every rb_host_*_text
entry point, with sentinel-filled outputs (tests/test_gpu_text_entry_points.py) -- and the oracle's answer for that batch.
tests/test_qbed_inputs.py holds these inputs to what the GPU tests say they contain, with the oracle alone."""
import ctypes as C
import zlib

import numpy as np

from rbtest_util import CONT, random_cigar, sums, unpack

LIFT_QBED = 1 << 21
E_INVALID = -1
F_STRIPPED = 2
GUARD = 0xDEADBEE5  # (code 5, 'H': no kernel here writes it)

# ---------------------------------------------------------------------------------------------- rb_dev_swap in place
# record lengths in words: the issue's list, and the sizes at which rb_k_swap_inplace takes another path -- a turn of 2 x 256 words runs
# while 512 or more words are left between the ends, what is left then (0 .. 511 words) is the middle
SWAP_LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1000, 1023, 1024, 1025,
                4097]


def plain_words(rng, n):
    """n words without continuation words: codes M I D = X, lengths 1 .. 2^28 - 1"""
    code = rng.choice([0, 1, 2, 7, 8], n, p=[.1, .25, .25, .3, .1]).astype(np.uint32)
    ln = rng.integers(1, 1 << 28, n).astype(np.uint32)
    return (ln << np.uint32(4)) | code


def with_pairs(rng, n, pairs, beside=None):
    """n words with an (owner, continuation) pair at every p, p + 1 of `pairs`; beside = (code in front of the pair, code behind it)"""
    w = plain_words(rng, n)
    for p in pairs:
        assert 0 <= p and p + 1 < n
        w[p] = (int(rng.integers(1, 1 << 28)) << 4) | int(rng.choice([0, 1, 2, 7]))  # the owner may itself be an I or a D: its code flips
        w[p + 1] = (int(rng.integers(1, 16)) << 4) | CONT
        if beside:
            if p > 0:
                w[p - 1] = (w[p - 1] & ~np.uint32(15)) | np.uint32(beside[0])
            if p + 2 < n:
                w[p + 2] = (w[p + 2] & ~np.uint32(15)) | np.uint32(beside[1])
    return w


# name -> (n words, pair positions, codes beside the pair)
PAIR_CASES = {
    "words 0-1": (10, [0], None),
    "words n-2..n-1": (10, [8], None),
    "straddles 63|64": (200, [63], None),
    "straddles the mirror of 63|64": (200, [200 - 65], None),
    "middle, odd n, below": (9, [3], None),
    "middle, odd n, above": (9, [4], None),
    "middle, even n": (10, [4], None),
    "two pairs back to back": (12, [3, 5], None),
    "one pair is the record": (2, [0], None),
    "beside I and D": (12, [5], (1, 2)),
    "beside D and I": (12, [5], (2, 1)),
    "both ends": (7, [0, 5], None),
    # the kernel's own edges: lanes hold 4 words (3|4), a turn's blocks are 256 words (255|256 and its mirror), turns end where the
    # middle begins (511|512 at n = 1300: two turns, a middle of 276 words held 64 to a register: 575|576), the middle's own centre
    "n 1300: lane, block, turn and middle edges": (1300, [3, 255, 511, 575, 649, 1300 - 513, 1300 - 257, 1300 - 5], None),
    "n 600: block | middle edges": (600, [255, 299, 343], None),
    "n 512: the two blocks meet": (512, [255], None),
    "n 513: one word between the blocks, pair in front": (513, [255], None),
    "n 513: one word between the blocks, pair behind": (513, [256], None),
    "n 1024: no middle": (1024, [255, 511, 767], None),
    "n 4097: every turn edge": (4097, list(range(255, 4097 - 2, 256)), None),
}


def swap_records():
    """[(what, words, strand)]: every length on both strands, every pair placement on both strands"""
    rng = np.random.default_rng(zlib.crc32(b"swap-inplace"))
    recs = []
    for n in SWAP_LENGTHS:
        w = plain_words(rng, n)
        recs += [(f"plain n={n} -", w, ord("-")), (f"plain n={n} +", w.copy(), ord("+"))]
    for what, (n, pairs, beside) in PAIR_CASES.items():
        w = with_pairs(rng, n, pairs, beside)
        recs += [(f"{what} -", w, ord("-")), (f"{what} +", w.copy(), ord("+"))]
    return recs


def pack_batch(recs, order, guard_front=5, guard_back=9):
    """the records of `order` back to back between guard words -> (whole array, op_off with op_off[0] = guard_front, strand)"""
    words = [recs[i][1] for i in order]
    off = np.zeros(len(order) + 1, np.uint64)
    off[0] = guard_front
    off[1:] = guard_front + np.cumsum([len(w) for w in words], dtype=np.uint64)
    arr = np.concatenate([np.full(guard_front, GUARD, np.uint32), *words, np.full(guard_back, GUARD, np.uint32)]).astype(np.uint32)
    return arr, off, np.array([recs[i][2] for i in order], np.uint8)


def swap_batches():
    """[(what, array, op_off, strand)]: all records in a shuffled order, and batches of 1, 3, 4 and 5 records (four waves per workgroup)"""
    recs = swap_records()
    rng = np.random.default_rng(zlib.crc32(b"swap-order"))
    out = [("all", *pack_batch(recs, rng.permutation(len(recs))))]
    minus = [i for i, r in enumerate(recs) if r[2] == ord("-") and len(r[1]) > 2]
    for k, gf in ((1, 4), (3, 5), (4, 6), (5, 7)):  # (the first record starts at every 16-byte phase)
        out.append((f"{k} records", *pack_batch(recs, rng.choice(minus, k, replace=False), guard_front=gf)))
    return out


def oracle_swap_whole(oracle, arr, off, strand):
    """the whole array as it must look after the swap: guards untouched, every record = oracle.swap"""
    z = np.zeros(len(strand), np.uint64)
    g = int(off[0])
    inner = arr[g:int(off[-1])]
    b = oracle.Batch(inner, off - np.uint64(g), z, z, z, z, strand)
    want = arr.copy()
    want[g:int(off[-1])] = oracle.swap(b)
    return want


# ---------------------------------------------------------------------------------------------- the RB_LIFT_QBED wrapper
def _rec(cig, q_name, q_st, strand, t_st, bad=0, bad_t=0):
    R, Q = sums(cig)
    return dict(cig=cig, q_name=q_name, q_st=q_st, q_en=q_st + Q + bad, t_st=t_st, t_en=t_st + R + bad + bad_t, strand=ord(strand))


def qbed_batch():
    """about 40 records (1 - 300 ops, two of about 3000), both strands, three query names interleaved, as read from a file; and about 30
    windows in QUERY coordinates.  -> dict(text, cig_off, cig_end, ops, op_off, t_st, t_en, q_st, q_en, strand, contig (of the QUERY names),
    w_contig, w_st, w_en, special = {what: record index})"""
    rng = np.random.default_rng(zlib.crc32(b"qbed-batch"))
    names = ["qA", "qB", "qC"]
    at = {n: 1000 for n in names}  # next free query position per name: records of one name do not overlap
    recs, special = [], {}

    def add(cig, strand, what=None, bad=0, name=None, bad_t=0):
        name = name or names[len(recs) % 3]
        r = _rec(np.asarray(cig, np.uint32), name, at[name], strand, int(rng.integers(0, 50_000)), bad, bad_t)
        at[name] = r["q_en"] + int(rng.integers(5, 400))
        if what:
            special[what] = len(recs)
        recs.append(r)

    op = lambda ln, c: (ln << 4) | "MIDNSHP=X".index(c)  # noqa: E731
    for i in range(30):
        n_ops = int(rng.choice([1, 2, 3, 7, 40, 150, 300]))
        add(random_cigar(rng, n_ops, "regular" if i % 4 else "indel_ends"), "+-"[int(rng.integers(0, 2))])
    add(random_cigar(rng, 3001, "regular"), "+", "long +")
    add(random_cigar(rng, 2950, "regular"), "-", "long -")
    add([op(30, "="), op(50, "I"), op(30, "=")], "+", "long insertion +")   # swapped: 50D -- a window inside it ends in an indel
    add([op(20, "="), op(40, "I"), op(25, "=")], "-", "long insertion -")
    add([op(10, "="), op(3, "D")], "-", "stripped -")                       # swapped and reversed: 3I10= -- stripped to 10=, id _TO.3I.
    add([op(4, "D"), op(12, "="), op(1, "X"), op(6, "=")], "+", "stripped +")
    add([op(15, "="), op(2, "X"), op(9, "=")], "+", "both spans off", bad=1)  # target span and query span both one longer than the CIGAR
    add(random_cigar(rng, 60, "regular"), "-")
    add(random_cigar(rng, 90, "regular"), "+")
    add([op(11, "="), op(2, "I"), op(8, "=")], "-", "target span off", bad_t=1)   # as read: the target check fails; swapped, it is the query check
    n = len(recs)
    cigs = [unpack(r["cig"]).encode() for r in recs]
    # the cg:Z: values as they lie in a file: other bytes between them
    text, cig_off, cig_end = b"", [], []
    for i, c in enumerate(cigs):
        text += b"x" * (i % 7 + 1)
        cig_off.append(len(text))
        text += c
        cig_end.append(len(text))
    text += b"\n" + b"\0" * 32
    op_off = np.zeros(n + 1, np.uint64)
    op_off[1:] = np.cumsum([len(r["cig"]) for r in recs])
    col = lambda k: np.array([r[k] for r in recs], np.uint64)  # noqa: E731
    ids = {nm: i for i, nm in enumerate(names)}
    d = dict(text=np.frombuffer(text, np.uint8).copy(), text_bytes=len(text) - 32, cig_off=np.array(cig_off, np.uint64), cig_end=np.array(cig_end, np.uint64),
             ops=np.concatenate([r["cig"] for r in recs]).astype(np.uint32), op_off=op_off, t_st=col("t_st"), t_en=col("t_en"), q_st=col("q_st"),
             q_en=col("q_en"), strand=np.array([r["strand"] for r in recs], np.uint8), contig=np.array([ids[r["q_name"]] for r in recs], np.uint32),
             special=special, q_names=[r["q_name"] for r in recs])
    # windows in query coordinates
    w = []
    for r in rng.choice(30, 12, replace=False):   # strictly inside a record, where it is long enough
        q0, q1 = recs[r]["q_st"], recs[r]["q_en"]
        if q1 - q0 >= 4:
            a = int(rng.integers(q0 + 1, q1 - 2))
            w.append((ids[recs[r]["q_name"]], a, int(rng.integers(a + 1, q1))))
    for r in list(rng.choice(30, 5, replace=False)) + [special["stripped -"], special["stripped +"]]:   # equal to a record's edges
        w.append((ids[recs[r]["q_name"]], recs[r]["q_st"], recs[r]["q_en"]))
    for r in (1, 2, 5):                             # a little wider than a record without end indels: the record comes back whole, INSIDE
        w.append((ids[recs[r]["q_name"]], recs[r]["q_st"] - 1, recs[r]["q_en"] + 2))
    for k in ("long +", "long -"):
        r = recs[special[k]]
        mid = (r["q_st"] + r["q_en"]) // 2
        w += [(ids[r["q_name"]], r["q_st"] + 17, mid), (ids[r["q_name"]], mid - 300, r["q_en"] - 3)]
    r = recs[special["long insertion +"]]
    w += [(ids[r["q_name"]], r["q_st"] + 40, r["q_st"] + 60), (ids[r["q_name"]], r["q_st"] + 10, r["q_st"] + 50)]   # inside the insertion; ending in it
    r = recs[special["long insertion -"]]
    w += [(ids[r["q_name"]], r["q_st"] + 30, r["q_st"] + 50), (ids[r["q_name"]], r["q_st"] + 35, r["q_st"] + 80)]
    r = recs[special["both spans off"]]
    w.append((ids[r["q_name"]], r["q_st"], r["q_en"]))
    w += [(3, 1000, 5000), (3, 0, 10)]              # a name no record has
    w += [(0, 900, at["qA"] + 10)]                  # one window over everything on qA: every record there lies inside it
    w.sort()
    d["w_contig"] = np.array([x[0] for x in w], np.uint32)
    d["w_st"], d["w_en"] = np.array([x[1] for x in w], np.uint64), np.array([x[2] for x in w], np.uint64)
    return d


def qbed_reference(oracle, d, policy=0):
    """what RB_LIFT_QBED must give, from the oracle: reduce rows of the batch as read; swap, normalize and liftover on the exchanged columns;
    the text of every row.  -> dict(red, swapped, norm, rows, out, text)"""
    as_read = oracle.Batch(d["ops"], d["op_off"], d["t_st"], d["t_en"], d["q_st"], d["q_en"], d["strand"])
    sw = oracle.swap(as_read)
    swapped = oracle.Batch(sw, d["op_off"], d["q_st"], d["q_en"], d["t_st"], d["t_en"], d["strand"], d["contig"])
    rows, out = oracle.liftover(swapped, d["w_contig"], d["w_st"], d["w_en"], policy)
    return dict(red=oracle.reduce(as_read), swapped=sw, norm=oracle.normalize(swapped), rows=rows, out=out, text=rows_text(rows, out))


def windows_without_stripped_inside(d, ref):
    """mask of the windows that leave no OK INSIDE row on a record whose end indels were stripped: with such a row
    rb_host_liftover_largest_text declines (the id _TO.<lead>.<trail> is no key)"""
    rows, norm = ref["rows"], ref["norm"]
    stripped = (norm["lead_ops"] + norm["trail_ops"]) > 0
    bad = (rows["status"] == 0) & ((rows["flags"] & 1) != 0) & stripped[rows["rec"]]
    keep = np.ones(len(d["w_st"]), bool)
    keep[rows["win"][bad]] = False
    return keep


def with_windows(d, keep):
    e = dict(d)
    for k in ("w_contig", "w_st", "w_en"):
        e[k] = np.ascontiguousarray(d[k][keep])
    return e


def rows_text(rows, out):
    """the CIGAR text of every oracle hit row (empty where the row is not OK)"""
    return [unpack(out[int(h["out_off"]):int(h["out_off"]) + int(h["out_n"])]).encode() if int(h["status"]) == 0 else b"" for h in rows]


# ---------------------------------------------------------------------------------------------- ctypes: the text wrappers
def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _take(L, ptr, n, dt):
    r = np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr.value), dtype=dt).copy() if n and ptr.value else np.zeros(0, dt)
    L.rb_host_free(ptr)
    return r


SENTINEL = 0xEE             # every caller-owned output is filled with this byte before a call, so "untouched" shows
UNTOUCHED = 0xEEEEEEEEEEEEEEEE  # ... and so is every out-pointer and *n_rows
INT_UNTOUCHED = -0x11111112  # (0xEEEEEEEE as an int)


def _filled(k, dt):
    return np.frombuffer(bytes([SENTINEL]) * (k * np.dtype(dt).itemsize), dt).copy()


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all())


def _text_call(eng, fn, d, policy, head, tail=(), form="text", null=()):
    """One call of a text entry point: the shared leading columns of `d`, the route's own `head` (contig + windows, max_size, or both), the
    shared outputs, the route's own `tail`.  form: "text" (row_text_off, row_text), "stats" (one reduce row per row in their place), "scan"
    (rb_host_scan_text: no policy, no rows).  null: names among rows / row_text_off / row_text / stats passed as NULL.
    -> dict(rc, error, cig_status, red, norm, counters, n_rows, ptr = {name: "null" | "untouched" | "set"}, rows, off, text, stats); rows, off
    (row_text_off: n_rows + 1 words, two of an empty result), text [bytes per row] and stats hold what the pointers gave (empty where they gave nothing)"""
    from rustybam_amd import capi
    n = len(d["strand"])
    st, red, norm, cnt = _filled(max(n, 1), np.uint8), _filled(n, capi.REDUCE_DT), _filled(n, capi.NORM_DT), _filled(1, capi.COUNTERS_DT)
    out = {k: C.c_void_p(UNTOUCHED) for k in ("rows", "row_text_off", "row_text", "stats")}
    ref = lambda k: C.c_void_p(0) if k in null else C.byref(out[k])  # noqa: E731
    nr = C.c_uint64(UNTOUCHED)
    last = {"text": ("row_text_off", "row_text"), "stats": ("stats",), "scan": ()}[form]
    outs = () if form == "scan" else (ref("rows"), C.byref(nr), *map(ref, last), _p(cnt))
    rc = fn(eng.ctx, C.c_uint64(n), _p(d["text"]), C.c_uint64(d["text_bytes"]), _p(d["cig_off"]), _p(d["cig_end"]), _p(d["t_st"]), _p(d["t_en"]),
            _p(d["q_st"]), _p(d["q_en"]), _p(d["strand"]), *head, *(() if form == "scan" else (C.c_int(policy),)), _p(st), _p(red), _p(norm),
            *outs, *tail)
    ptr = {k: "null" if p.value is None else "untouched" if p.value == UNTOUCHED else "set" for k, p in out.items()}
    r = dict(rc=int(rc), error=eng.L.rb_ctx_last_error(eng.ctx).decode() if rc != 0 else "", cig_status=st[:n], red=red, norm=norm,
             counters=cnt, n_rows=int(nr.value), ptr=ptr)
    k = r["n_rows"] if rc == 0 and r["n_rows"] != UNTOUCHED else 0
    take = lambda key, m, dt: _take(eng.L, out[key], m, dt) if ptr[key] == "set" else np.zeros(0, dt)  # noqa: E731
    r["off"] = off = take("row_text_off", max(k + 1, 2), np.uint64)  # (an empty result still has two words)
    txt = take("row_text", int(off[k]) if k and len(off) > k else 0, np.uint8).tobytes()
    r["rows"], r["stats"] = take("rows", k, capi.HIT_DT), take("stats", k, capi.REDUCE_DT)
    r["text"] = [txt[int(off[i]):int(off[i + 1])] for i in range(k)] if len(off) > k else []
    return r


def _windows(d):
    return (_p(d["contig"]), C.c_uint64(len(d["w_st"])), _p(d["w_contig"]), _p(d["w_st"]), _p(d["w_en"]))


# the text entry points: name -> (form, what stands between the columns and the policy, what stands behind the counters)
TEXT_ENTRY_POINTS = {
    "rb_host_liftover_text": ("text", "windows", None),
    "rb_host_liftover_largest_text": ("text", "windows", "largest"),
    "rb_host_liftover_stats_text": ("stats", "windows", None),
    "rb_host_break_text": ("text", "max_size", None),
    "rb_host_break_stats_text": ("stats", "max_size", None),
    "rb_host_break_pairs_text": ("text", "max_size", "pairs"),
    "rb_host_break_pairs_stats_text": ("stats", "max_size", "pairs"),
    "rb_host_break_liftover_text": ("text", "both", "pieces"),
    "rb_host_break_liftover_stats_text": ("stats", "both", "pieces"),
    "rb_host_scan_text": ("scan", None, None),
}


def text_entry(eng, name, d, policy=0, max_size=10, largest=None, pairs=None, null=()):
    """Entry point `name` on the batch `d` (text, text_bytes, cig_off, cig_end, the columns, contig, w_contig, w_st, w_en).
    largest = (win_key, n_keys, inside_key); pairs = dict(rec_key, rec_q_len, n_keys, mode, paired_len, min_aln, min_query).
    -> what _text_call gives, and declined / key_flip / row_piece (None: NULL, "untouched", or the pieces) where the entry point has them"""
    form, mid, end = TEXT_ENTRY_POINTS[name]
    head = {"windows": lambda: _windows(d), "max_size": lambda: (C.c_uint32(max_size),), "both": lambda: (*_windows(d), C.c_uint32(max_size)),
            None: lambda: ()}[mid]()
    declined, piece, key_flip, keep = C.c_int(INT_UNTOUCHED), C.c_void_p(UNTOUCHED), None, []
    tail = ()
    if end == "largest":
        keep = [np.ascontiguousarray(largest[0], np.uint32)]
        tail = (_p(keep[0]), C.c_uint64(largest[1]), C.c_uint32(largest[2]), C.byref(declined))
    elif end == "pairs":
        keep = [np.ascontiguousarray(pairs["rec_key"], np.uint32), np.ascontiguousarray(pairs["rec_q_len"], np.uint64)]
        key_flip = _filled(pairs["n_keys"] + 1, np.uint8)
        tail = (_p(keep[0]), _p(keep[1]), C.c_uint64(pairs["n_keys"]), C.c_uint32(pairs["mode"]), C.c_uint64(pairs.get("paired_len", 0)),
                C.c_uint64(pairs.get("min_aln", 0)), C.c_uint64(pairs.get("min_query", 0)), _p(key_flip), C.byref(declined))
    elif end == "pieces":
        tail = (C.byref(piece), C.byref(declined))
    r = _text_call(eng, getattr(eng.L, name), d, policy, head, tail, form, null)
    if end:
        r["declined"] = declined.value
    if end == "pairs":
        r["key_flip"] = key_flip[:pairs["n_keys"]]
    if end == "pieces":
        r["row_piece"] = None if piece.value is None else "untouched" if piece.value == UNTOUCHED else _take(eng.L, piece, len(r["rows"]), np.uint32)
    return r


def text_batch(cigars, t_st, q_st, strands, contig, windows):
    """records with the CIGAR strings `cigars` (they need not parse) as they lie in a file, other bytes between the values; the spans are
    those of whatever ops the strings hold.  windows: [(contig, st, en)] -> the dict text_entry takes, with ops / op_off for the oracle"""
    from rbtest_util import pack
    ops = [pack(c) for c in cigars]
    text, cig_off, cig_end = b"", [], []
    for i, c in enumerate(cigars):
        text += b"x" * (i % 7 + 1)
        cig_off.append(len(text))
        text += c.encode()
        cig_end.append(len(text))
    text += b"\n" + b"\0" * 32
    span = [sums(o) if len(o) else (0, 0) for o in ops]
    u64 = lambda x: np.array(x, np.uint64)  # noqa: E731
    op_off = np.zeros(len(ops) + 1, np.uint64)
    op_off[1:] = np.cumsum([len(o) for o in ops])
    return dict(text=np.frombuffer(text, np.uint8).copy(), text_bytes=len(text) - 32, cig_off=u64(cig_off), cig_end=u64(cig_end),
                ops=np.concatenate(ops).astype(np.uint32) if ops else np.zeros(0, np.uint32), op_off=op_off, t_st=u64(t_st),
                t_en=u64([a + s[0] for a, s in zip(t_st, span)]), q_st=u64(q_st), q_en=u64([a + s[1] for a, s in zip(q_st, span)]),
                strand=np.array([ord(s) for s in strands], np.uint8), contig=np.array(contig, np.uint32),
                w_contig=np.array([w[0] for w in windows], np.uint32), w_st=u64([w[1] for w in windows]), w_en=u64([w[2] for w in windows]))


def host_liftover_text(eng, d, policy):
    """rb_host_liftover_text on the batch of qbed_batch() -> dict(rc, cig_status, red, norm, rows, text [bytes per row]) or dict(rc, error)"""
    return _text_call(eng, eng.L.rb_host_liftover_text, d, policy, _windows(d))


def host_liftover_largest_text(eng, d, policy, win_key, n_keys, inside_key):
    declined = C.c_int(-1)
    wk = np.ascontiguousarray(win_key, np.uint32)
    r = _text_call(eng, eng.L.rb_host_liftover_largest_text, d, policy, _windows(d), (_p(wk), C.c_uint64(n_keys), C.c_uint32(inside_key), C.byref(declined)))
    r["declined"] = declined.value
    return r


def host_break_text(eng, d, policy, max_size=10):
    return _text_call(eng, eng.L.rb_host_break_text, d, policy, (C.c_uint32(max_size),))
