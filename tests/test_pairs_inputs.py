"""The inputs of tests/test_gpu_pairs_rows.py hold what they are named for, the numpy model (tests/pairs_util.py) says what the oracle's
`break-paf | orient | filter` pipeline says, and rb_host_pairs_rows -- the library's plain C++ statement of the same rules -- agrees with the
model byte for byte.  No GPU."""
import os

import numpy as np
import pytest

import pairs_util as pu
import rustybam_amd
from rustybam_amd import capi

NEW_SYMBOLS = ["rb_dev_pairs_rows", "rb_host_pairs_rows", "rb_pairs_scratch_bytes", "rb_pairs_shape", "rb_host_break_pairs_text",
               "rb_host_break_pairs_stats_text"]


def test_the_library_exports_the_new_names():
    assert set(NEW_SYMBOLS) <= set(rustybam_amd.declared_symbols())
    assert set(NEW_SYMBOLS) <= set(rustybam_amd.exported_symbols())
    wave_rows, block_rows = capi.pairs_shape()
    assert wave_rows % 64 == 0 and block_rows == 4 * wave_rows
    f = capi.lib().rb_pairs_scratch_bytes
    f.restype = capi.C.c_size_t
    assert f(capi.C.c_uint64(0), capi.C.c_uint64(0)) > 0 and f(capi.C.c_uint64(9), capi.C.c_uint64(2447)) >= 3 * 9 * 8 + 2448 * 8


CASES = pu.all_cases()


def same(got, m, what, rows_cap=None):
    rows_out, key_flip, info = got
    n = len(m.rows_out) if rows_cap is None else min(len(m.rows_out), rows_cap)
    assert info.tobytes() == pu.model_info(m, rows_cap).tobytes(), f"{what}: info {info} != {pu.model_info(m, rows_cap)}"
    assert key_flip.tobytes() == m.key_flip.tobytes(), f"{what}: key_flip"
    assert rows_out.tobytes() == m.rows_out[:n].tobytes(), f"{what}: rows_out"


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_host_mirror_is_the_model(c):
    for mode in (c.mode, 0, pu.ORIENT, pu.FILTER, pu.ORIENT | pu.FILTER):
        m = pu.model(c, mode)
        same(capi.host_pairs_rows(c.rows, c.rec_key, c.rec_q_len, c.strand, c.n_keys, mode, c.L, c.A, c.Q), m, f"{c.name}, mode {mode}")
    m = pu.model(c)
    for cap in {0, 1, max(len(m.rows_out) - 1, 0)}:
        same(capi.host_pairs_rows(c.rows, c.rec_key, c.rec_q_len, c.strand, c.n_keys, c.mode, c.L, c.A, c.Q, rows_cap=cap), m, f"{c.name}, rows_cap {cap}", cap)


def test_row_counts():
    wave_rows, block_rows = capi.pairs_shape()
    counts = pu.row_counts()
    assert {0, 1, 63, 64, 65, 255, 256, 257, block_rows + 1} <= set(counts)
    for n in counts:
        c = pu.random_case(n, 100 + n)
        m = pu.model(c)
        assert len(c.rows) == n
        if n >= 255:  # every path is populated: rows of another status, rows dropped by each test, both kinds of key, several runs per wavefront
            ok = c.rows["status"] == 0
            assert 0 < (~ok).sum() < n / 5 and 0 < m.info["n_kept"] < ok.sum() and 0 < m.info["n_flipped_rows"] <= m.info["n_kept"]
            assert 0 < m.key_flip.sum() < c.n_keys and (np.diff(m.key[:64]) != 0).sum() >= 2


@pytest.mark.parametrize("c", pu.key_run_cases(), ids=lambda c: c.name)
def test_key_runs(c):
    m, e = pu.model(c), c.expect
    if "run" in e:
        start, run = e["run"]
        k1 = np.nonzero(m.key == 1)[0]
        assert (k1[0], len(k1)) == (start, run) and (np.diff(k1) == 1).all(), "key 1 is one run of that length at that lane"
        assert (int(m.orient[1]), int(m.fspan[1]), int(m.key_flip[1])) == (e["orient1"], e["fspan1"], e["flip1"])
        assert int((m.keep & (m.key == 1)).sum()) == e["kept1"] and c.L in (e["fspan1"], e["fspan1"] - 1)
        part1 = m.part & (m.key == 1)
        assert part1.sum() == e["fspan1"] // 10
        if "cut" in c.name:  # rows of another status inside the run: in no sum, not in rows_out
            cut = (m.key == 1) & ~m.part
            assert cut.sum() == 5 and cut[start] and cut[start + 128] and not m.keep[cut].any()
            assert set(c.rows["win"][cut].tolist()).isdisjoint(m.rows_out["win"].tolist())
    if "key_flip" in e:
        assert m.key_flip.tolist() == e["key_flip"]
    if "kept" in e:
        assert int(m.info["n_kept"]) == e["kept"]
    if c.name == "all keys distinct":
        assert len(np.unique(m.key)) == len(c.rows) == c.n_keys and 0 < m.info["n_kept"] < len(c.rows) and 0 < m.key_flip.sum() < c.n_keys
    if c.name == "ABAB":
        assert (np.diff(m.key) != 0).all()
    if c.name.startswith("one key"):
        assert (m.key == 1).all() and len(c.rows) == 700 > capi.pairs_shape()[0]


@pytest.mark.parametrize("c", pu.threshold_cases() + pu.wide_cases() + pu.decline_cases(), ids=lambda c: c.name)
def test_thresholds_sums_and_declines(c):
    m, e = pu.model(c), c.expect
    assert e, "every one of these cases says what it expects"
    if "key_flip" in e:
        assert m.key_flip.tolist() == e["key_flip"]
    if "kept" in e:
        assert int(m.info["n_kept"]) == e["kept"]
    if "declined" in e:
        assert int(m.info["declined"]) == e["declined"]
        if e["declined"]:  # ... with the other rows of the call still well-formed
            assert m.info["n_kept"] > 0
    if c.name.startswith("orient sum"):
        want = {"orient sum 0": 0, "orient sum -1": -1, "orient sum +1": 1}.get(c.name)
        if want is not None:
            assert int(m.orient[0]) == want
    if c.name == "a row that fails A does not count":
        assert int(m.fspan[0]) == 50 < c.L < int(m.tspan[0]) == 60
    if c.name == "a row that fails Q does not count":
        assert int(m.fspan[0]) == 30 < c.L < int(m.tspan[0]) == 60
    if c.name.startswith("span sum past 2^32"):
        assert int(m.fspan[0]) == 6_000_000_005 > 1 << 32 and c.rows["t_st"].min() < 1 << 32 < c.rows["t_en"].max()
    if c.name.startswith("orient sums"):
        assert sorted(abs(int(x)) for x in m.orient) == [(1 << 32) + 22] * 2
    if c.name == "orient sum through -2^32 and back to +1":
        assert int(m.orient[0]) == 1


def test_each_mode_bit():
    cs = {c.name: pu.model(c) for c in pu.mode_cases()}
    ok = int((pu.mode_cases()[0].rows["status"] == 0).sum())
    o, f, b, n = (cs[f"mode: {k}"] for k in ("orient only", "filter only", "both", "neither"))
    assert o.info["n_kept"] == ok and o.info["n_flipped_rows"] > 0, "orient only: nothing dropped"
    assert f.info["n_flipped_rows"] == 0 and not f.key_flip.any() and 0 < f.info["n_kept"] < ok, "filter only: nothing flipped"
    assert b.info["n_kept"] == f.info["n_kept"] and 0 < b.info["n_flipped_rows"] < o.info["n_flipped_rows"]
    c = pu.mode_cases()[3]
    assert n.rows_out.tobytes() == c.rows[c.rows["status"] == 0].tobytes(), "neither: a plain compaction of the OK rows"


# ---- the model against the oracle's own commands, piped together ----
# pieces, flipped rows under orient and rows kept at --paired-len 1000000 of the oracle's pipeline on asm_small.paf, by --max-size
COUNTS = {100: (2447, 978, 1944), 1000: (553, 172, 525), 5000: (280, 144, 269), 0: (46935, 7576, 43915)}


@pytest.mark.parametrize("max_size", list(COUNTS))
def test_model_reproduces_the_oracle_pipeline(oracle, golden, max_size):
    paf = os.path.join(golden, "asm_small.paf")
    R = pu.asm_small_recs()
    b, rec_key, q_len, n_keys = pu.asm_small()
    assert n_keys == 9
    rows, _ = oracle.break_paf(oracle.Batch(*R.arrays(), R.contig), max_size)
    rows = capi.hit_rows_from(rows)
    rc, pieces = oracle.cli("break-paf", "--max-size", max_size, paf)
    assert rc == 0 and pieces.count(b"\n") == int((rows["status"] == 0).sum()) == COUNTS[max_size][0]
    c = pu.case("asm_small", rows, rec_key, q_len, R.strand, n_keys)
    for mode, L in ((pu.ORIENT, 0), (pu.FILTER, 1_000_000), (pu.ORIENT | pu.FILTER, 1_000_000), (pu.FILTER, 0), (pu.ORIENT | pu.FILTER, 10_000)):
        c.L = L
        m = pu.model(c, mode)
        out = pieces
        if mode & pu.ORIENT:
            rc, out = oracle.cli("orient", "-", stdin=out)
            assert rc == 0
        if mode & pu.FILTER:
            rc, out = oracle.cli("filter", "--paired-len", L, "-", stdin=out)
            assert rc == 0
        lines = out.decode().splitlines()
        assert len(lines) == int(m.info["n_kept"]) and m.info["declined"] == 0
        if mode == pu.ORIENT:
            assert (len(lines), int(m.info["n_flipped_rows"]), int(m.key_flip.sum())) == (COUNTS[max_size][0], COUNTS[max_size][1], 5)
        elif L == 1_000_000:
            assert len(lines) == COUNTS[max_size][2]
        else:
            assert len(lines) == COUNTS[max_size][0], "L of 0 and 10000 keep everything"
        for ln, h in zip(lines, m.rows_out):
            t, r = ln.split("\t"), int(h["rec"])
            flip = bool(m.key_flip[rec_key[r]])
            sfx = ("-" if flip else "+") if mode & pu.ORIENT else ""
            strand = chr(R.strand[r]) if not flip else ("-" if chr(R.strand[r]) == "+" else "+")
            assert (t[0], int(t[2]), int(t[3]), t[4], t[5], int(t[7]), int(t[8]), t[12]) == \
                (R.q_name[r] + sfx, int(h["q_st"]), int(h["q_en"]), strand, R.t_name[r], int(h["t_st"]), int(h["t_en"]), "id:Z:"), ln[:100]
