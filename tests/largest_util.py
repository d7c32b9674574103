"""liftover --largest (main.rs:200-208) as a plain reference over hit rows, and the fabricated row sets of tests/test_gpu_largest.py.

main.rs:200-208, with `new_recs` the records trim_paf_by_rgns returned:

    new_recs.sort_by(|a, b| a.id.cmp(&b.id));                       // stable
    for (_key, group) in &new_recs.into_iter().group_by(|x| x.id.clone()) {
        let largest = group.max_by_key(|x| x.t_en - x.t_st).unwrap();   // max_by_key: the LAST maximum
        println!("{}", largest);
    }

Hit rows stand for new_recs: they are in its order, a row whose status is not 0 is a pair the reference dropped, and the id of a row is
a key -- rec_key[rec] for a record that lies inside its window (HIT_INSIDE, liftover.rs:23-25), win_key[win] otherwise.  Keys number the
id strings in ascending bytewise order, so sorting by key is sorting by id."""
import numpy as np

from rustybam_amd.capi import HIT_DT, HIT_INSIDE

ST_OK, ST_NONE_INDEL, ST_NONE_EMPTY = 0, 1, 3
BAD_KEY = 0xFFFFFFFF


def row_keys(rows, win_key, rec_key):
    """key of every row as an int64 array (rows that are not OK included: the reference never asks for theirs); -1 where an INSIDE row
    has no rec_key to take"""
    win_key = np.asarray(win_key, np.int64)
    inside = (rows["flags"].astype(np.int64) & HIT_INSIDE) != 0
    k = win_key[rows["win"].astype(np.int64)] if len(rows) else np.zeros(0, np.int64)
    if rec_key is None:
        return np.where(inside, -1, k)
    return np.where(inside, np.asarray(rec_key, np.int64)[rows["rec"].astype(np.int64)], k)


def spans(rows):
    return rows["t_en"].astype(np.uint64) - rows["t_st"].astype(np.uint64)


def largest_ref(rows, win_key, rec_key, n_keys):
    """-> (sel: the row index printed for every id, in id order, u64; n_bad: OK rows whose key is not one of the n_keys)"""
    key, span = row_keys(rows, win_key, rec_key), spans(rows)
    ok = rows["status"].astype(np.int64) == ST_OK
    good = ok & (key >= 0) & (key < n_keys)
    new_recs = [(int(key[k]), int(span[k]), int(k)) for k in np.nonzero(good)[0]]   # (id, t_en - t_st, where it came from)
    new_recs.sort(key=lambda r: r[0])                                                  # list.sort is stable, as sort_by is
    sel, i = [], 0
    while i < len(new_recs):
        j, best = i, new_recs[i]
        while j < len(new_recs) and new_recs[j][0] == new_recs[i][0]:                  # group_by
            if new_recs[j][1] >= best[1]:                                              # max_by_key keeps the last maximum
                best = new_recs[j]
            j += 1
        sel.append(best[2])
        i = j
    return np.array(sel, np.uint64), int((ok & ~good).sum())


def intern_ids(ids):
    """-> (key of every id in `ids`, key of the empty id, number of keys): the ids and "" numbered in ascending bytewise order"""
    table = sorted({i.encode() for i in ids} | {b""})
    pos = {s: k for k, s in enumerate(table)}
    return np.array([pos[i.encode()] for i in ids], np.uint32), pos[b""], len(table)


def repeated_id_bed(path):
    """the 100 kb tiling of the fixture's contigs with a column 4 that repeats: several windows share an id, and the ids sort differently
    by byte and by letter"""
    from golden.make_digests import tile_bed
    tile_bed(path)
    names = ["a", "B", "Z", "a1", "_x"]
    lines = [ln.rstrip("\n") for ln in open(path)]
    with open(path, "w") as f:
        for i, ln in enumerate(lines):
            f.write(f"{ln}\t{names[i % len(names)]}\n")


# ------------------------------------------------------------------ fabricated rows
def make_rows(recs, wins, status, flags, span, t_st=None):
    n = len(recs)
    rows = np.zeros(n, HIT_DT)
    rows["rec"], rows["win"], rows["status"], rows["flags"] = recs, wins, status, flags
    rows["t_st"] = np.arange(n, dtype=np.uint64) * np.uint64(3) if t_st is None else t_st
    rows["t_en"] = rows["t_st"] + np.asarray(span, np.uint64)
    rows["out_n"], rows["out_off"] = 1, np.arange(n, dtype=np.uint64) * np.uint64(4)   # (not read by rb_dev_largest)
    return rows


def one_key(n):
    """n rows, all on one key, all spans equal: the winner is the last row"""
    return dict(rows=make_rows(np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.full(n, 77)), win_key=np.array([0], np.uint32),
                rec_key=np.array([0], np.uint32), n_keys=1)


def contended(seed=5, n=20_000):
    """one key, random spans out of few values: every lane of every wave goes for one address, and the maximum is tied many times"""
    rng = np.random.default_rng(seed)
    return dict(rows=make_rows(np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), rng.integers(0, 40, n)), win_key=np.array([0], np.uint32),
                rec_key=np.array([0], np.uint32), n_keys=1)


def sparse(seed=6, n=5_000, n_keys=70_001):
    """few rows over many keys: most keys have no row; the first and the last key have one, so has every boundary of the scan's blocks of
    2048 keys on one side or the other"""
    rng = np.random.default_rng(seed)
    edge = np.arange(2048, n_keys, 2048)
    keys = np.concatenate([[0, n_keys - 1], edge, edge - 1, rng.integers(0, n_keys, n - 2 - 2 * len(edge))])
    rng.shuffle(keys)
    wk = np.arange(n_keys, dtype=np.uint32)          # window w has key w
    return dict(rows=make_rows(np.zeros(n), keys, np.zeros(n), np.zeros(n), rng.integers(0, 1000, n)), win_key=wk, rec_key=np.array([0], np.uint32),
                n_keys=n_keys)


def properties():
    """every case the selection can get wrong, by hand; window w has key w (w = 8, 9: keys outside the 8), record r has key REC_KEY[r]"""
    REC_KEY = [4, 4, 0, 12]
    I = HIT_INSIDE
    t = [  # (rec, win, status, flags, span)
        (0, 3, ST_OK, 0, 0),                     # row 0, key 3: its only OK row, of span 0 (pass 2's + 1; nothing for pass 1 to store)
        (0, 0, ST_OK, 0, 10), (1, 0, ST_OK, 0, 50), (2, 0, ST_OK, 0, 50), (0, 0, ST_OK, 0, 50), (1, 0, ST_OK, 0, 7),   # key 0: three rows tied at 50
        (0, 1, ST_OK, 0, 5), (1, 1, ST_NONE_INDEL, 0, 1000), (2, 1, ST_OK, 0, 9), (0, 1, ST_OK, 0, 2),               # key 1: the largest span is not OK
        (0, 2, ST_NONE_EMPTY, 0, 30), (1, 2, ST_NONE_INDEL, 0, 40),                                                    # key 2: no OK row
        (3, 3, ST_NONE_INDEL, 0, 8),                                                                                   # (key 3 again, not OK)
        (0, 0, ST_OK, I, 1 << 20), (1, 0, ST_OK, I, 1 << 21), (1, 5, ST_OK, I, 3),     # INSIDE: rec_key says key 4; their windows say keys 0 and 5
        ((2), 7, ST_OK, I, 6),                                                         # INSIDE on record 2: key 0, below its maximum
        (0, 5, ST_OK, 0, (1 << 32) + 5), (1, 5, ST_OK, 0, 7), (2, 5, ST_OK, 0, 0xFFFFFFFF),                           # key 5: a span >= 2^32
        (0, 6, ST_OK, 0, (1 << 33) + 123), (1, 6, ST_OK, 0, (1 << 32) + 123), (2, 6, ST_OK, 0, 123),                   # key 6: equal low halves
        (0, 8, ST_OK, 0, 99), (1, 9, ST_OK, 0, 1 << 40), (3, 1, ST_OK, I, 17),         # keys 8, 9 and record 3's key 12: outside the key space
        (0, 9, ST_NONE_INDEL, 0, 5),                                                   # (not OK: not looked at, not counted)
    ]                                                                                  # key 7: no row at all
    a = np.array([[int(x) for x in r] for r in t], dtype=object)
    rows = make_rows(a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint16), a[:, 3].astype(np.uint16),
                     np.array([int(x) for x in a[:, 4]], np.uint64), t_st=np.arange(len(t), dtype=np.uint64) * np.uint64(1000))
    return dict(rows=rows, win_key=np.arange(10, dtype=np.uint32), rec_key=np.array(REC_KEY, np.uint32), n_keys=8)


def skewed(seed, n=50_000, n_keys=500, n_rec=300):
    """random rows: one key takes half of them, 10 % are not OK, 10 % are INSIDE (records' keys are spread like the windows'), spans tie"""
    rng = np.random.default_rng(seed)
    n_win = 2 * n_keys
    wk = rng.integers(0, n_keys, n_win).astype(np.uint32)
    hot = int(wk[0])
    wk[rng.random(n_win) < 0.02] = n_keys + 5                                    # a few windows outside the key space
    win = np.where(rng.random(n) < 0.5, 0, rng.integers(0, n_win, n))
    rk = np.where(rng.random(n_rec) < 0.5, hot, rng.integers(0, n_keys + 2, n_rec)).astype(np.uint32)
    status = np.where(rng.random(n) < 0.1, rng.choice([1, 2, 3, 4, 5], n), 0)
    flags = np.where(rng.random(n) < 0.1, HIT_INSIDE, 0) | np.where(rng.random(n) < 0.3, 2, 0)   # (HIT_GENERIC: informational, no part in it)
    span = np.where(rng.random(n) < 0.2, rng.integers(1 << 32, (1 << 32) + 6, n), rng.integers(0, 12, n))
    return dict(rows=make_rows(rng.integers(0, n_rec, n), win, status, flags, span), win_key=wk, rec_key=rk, n_keys=n_keys)
