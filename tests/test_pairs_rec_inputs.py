"""The inputs of tests/test_gpu_pairs_records.py and tests/test_gpu_cli_orient_filter.py hold what they are named for, the numpy model
(tests/pairs_rec_util.py) says what the oracle's `orient`, `orient --scaffold -i I` and `filter` print, and rb_host_pairs_records -- the
library's plain C++ statement of the same rules -- agrees with the model byte for byte.  No GPU."""
import numpy as np
import pytest

import pairs_rec_util as pr
import rustybam_amd
from rustybam_amd import capi

NEW_SYMBOLS = ["rb_dev_pairs_records", "rb_host_pairs_records", "rb_pairs_records_scratch_bytes", "rb_pairs_records_shape", "rb_host_pairs_text"]


def test_the_library_exports_the_new_names():
    assert set(NEW_SYMBOLS) <= set(rustybam_amd.declared_symbols())
    assert set(NEW_SYMBOLS) <= set(rustybam_amd.exported_symbols())
    W, B = capi.pairs_records_shape()
    assert W % 64 == 0 and W > 64 and B == 4 * W
    f = capi.lib().rb_pairs_records_scratch_bytes
    f.restype = capi.C.c_size_t
    assert f(capi.C.c_uint64(0), capi.C.c_uint64(0)) > 0 and f(capi.C.c_uint64(9), capi.C.c_uint64(2447)) >= 4 * 9 * 8 + 2448 * 8


CASES = pr.all_cases()


def same(got, m, what, kept_cap=None):
    n = len(m.kept) if kept_cap is None else min(len(m.kept), kept_cap)
    want = pr.model_info(m, kept_cap)
    assert got["info"].tobytes() == want.tobytes(), f"{what}: info {got['info']} != {want}"
    for k in ("key_flip", "key_order", "q_st", "q_en"):
        assert got[k].tobytes() == getattr(m, k).tobytes(), f"{what}: {k}"
    assert got["kept"].tobytes() == m.kept[:n].tobytes(), f"{what}: kept"


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_host_mirror_is_the_model(c):
    for mode in (c.mode, 0, pr.ORIENT, pr.FILTER, pr.ORIENT | pr.FILTER):
        same(capi.host_pairs_records(*pr.columns(c), c.n_keys, mode, c.L, c.A, c.Q), pr.model(c, mode), f"{c.name}, mode {mode}")
    m = pr.model(c)
    for cap in {0, 1, max(len(m.kept) - 1, 0)}:
        same(capi.host_pairs_records(*pr.columns(c), c.n_keys, c.mode, c.L, c.A, c.Q, kept_cap=cap), m, f"{c.name}, kept_cap {cap}", cap)


def test_host_mirror_refuses():
    c = pr.random_case(10, 1)
    with pytest.raises(rustybam_amd.RbError):
        capi.host_pairs_records(*pr.columns(c), c.n_keys, 4)


def test_record_counts():
    W, B = pr.shape()
    counts = pr.record_counts()
    assert counts == [0, 1, 63, 64, 65, W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 7] and max(counts) < 5000
    for n in counts:
        c = pr.random_case(n, 100 + n)
        m = pr.model(c)
        assert len(c.t_st) == n and m.info["declined"] == 0
        if n >= 63:
            assert 0 < m.info["n_kept"] < n and 0 < pr.model(c, pr.ORIENT).info["n_flipped_rows"] < n
        if n >= W - 1:  # every path is populated: records dropped by each test, both kinds of key, several runs per group of 64
            assert m.info["n_flipped_rows"] < m.info["n_kept"] and 0 < m.key_flip.sum() < c.n_keys and (np.diff(c.rec_key[:64].astype(np.int64)) != 0).sum() >= 2
            assert (~m.passes).any() and (m.passes & ~m.keep).any() and (m.key_order != 0).all()


@pytest.mark.parametrize("c", pr.layout_cases(), ids=lambda c: c.name)
def test_layouts(c):
    W, B = pr.shape()
    m, e, key = pr.model(c), c.expect, c.rec_key.astype(np.int64)
    if "run" in e:
        start, run = e["run"]
        k1 = np.nonzero((key == 1) | (key == 3))[0]
        assert (k1[0], len(k1)) == (start, run) and (np.diff(k1) == 1).all(), "key 1 is one run of that length at that lane"
        assert (int(m.orient[1]), int(m.fspan[1]), int(m.key_flip[1])) == (e["orient1"], e["fspan1"], e["flip1"])
        assert int((m.keep & (key == 1)).sum()) == e["kept1"] and c.L in (e["fspan1"], e["fspan1"] - 1)
        if "cut" in c.name:  # records outside the key space inside the run: in no sum, not kept, and the call declines for them
            cut = key == 3
            assert cut.sum() == 5 and cut[start] and cut[start + 128] and not m.keep[cut].any() and not m.part[cut].any()
            assert m.info["declined"] == pr.DECL_KEY and int((m.part & (key == 1)).sum()) == e["fspan1"] // 10 == run - 5
        else:
            assert m.info["declined"] == 0
    if c.name.startswith("one key"):
        assert (key == 1).all() and len(key) > W + 64
    if c.name == "every record its own key":
        assert len(np.unique(key)) == len(key) == c.n_keys and 0 < m.info["n_kept"] < len(key) and 0 < m.key_flip.sum() < c.n_keys
    if c.name == "two keys alternating":
        assert (np.diff(key) != 0).all() and set(key) == {0, 1} and len(key) > B and m.info["n_kept"] > 0
    if "cuts" in e:
        ends = np.nonzero(np.diff(key) != 0)[0]          # the last record of every run but the last
        lens = np.diff(np.concatenate([[-1], ends, [len(key) - 1]]))
        assert lens.min() == 1 and lens.max() == 130 and len(key) > 2 * B
        lanes = set((ends % 64).tolist())
        assert {62, 63, 0} <= lanes, "a run ends at lane 62, at lane 63 (on a group boundary) and at lane 0"
        assert W - 1 in ends and B - 1 in ends and 2 * B - 1 in ends and B + W - 1 in ends, "... and on a wavefront's and a workgroup's boundary"
        assert B in ends and W in ends, "... and a run of one record begins a wavefront and a workgroup"
        assert 0 < m.info["n_kept"] < len(key) and 0 < m.key_flip.sum() < c.n_keys and c.n_keys == 41 < len(lens)


@pytest.mark.parametrize("c", pr.threshold_cases() + pr.wide_cases() + pr.decline_cases(), ids=lambda c: c.name)
def test_thresholds_sums_and_declines(c):
    m, e = pr.model(c), c.expect
    assert e, "every one of these cases says what it expects"
    for k in ("key_flip", "orient", "tspan", "fspan"):
        if k in e:
            assert [int(x) for x in getattr(m, k)] == e[k], k
    if "kept" in e:
        assert int(m.info["n_kept"]) == e["kept"]
    if "declined" in e:
        assert int(m.info["declined"]) == e["declined"]
    if c.name.startswith("spans of 2^62"):
        assert int((c.t_en - c.t_st).min()) == 1 << 62
    if c.name == "spans of 2^62: five records":
        exact = sum(((1 << 62) * (2 * int(t) + (1 << 62))) % (1 << 64) // 2 for t in c.t_st)
        assert exact >= 1 << 64, "the order sum wraps, after products that wrapped"
        assert int(m.key_order[0]) == exact % (1 << 64) // (1 << 62) and m.q_st.tolist() == [int(c.rec_q_len[r] - c.q_en[r]) for r in range(5)]
    if "fails" in c.name:
        assert not m.passes[0] and m.part[0] and m.flip[0], "the record that fails the filter is the one that flips the key"
    if c.name.startswith("declines: q_len"):
        assert int(m.q_st[1]) == (104 - 105) % (1 << 64), "the wrapped value is still what comes out"


def test_each_mode_bit():
    n_, o, f, b = (pr.model(c) for c in pr.mode_cases())
    n = len(pr.mode_cases()[0].t_st)
    assert [c.mode for c in pr.mode_cases()] == [0, 1, 2, 3]
    assert n_.info["n_kept"] == n and not n_.key_flip.any() and not n_.key_order.any() and n_.info["n_flipped_rows"] == 0
    assert o.info["n_kept"] == n and o.info["n_flipped_rows"] > 0 and o.key_order.all(), "orient only: nothing dropped"
    assert f.info["n_flipped_rows"] == 0 and not f.key_flip.any() and not f.key_order.any() and 0 < f.info["n_kept"] < n, "filter only: nothing flipped"
    assert b.info["n_kept"] == f.info["n_kept"] and 0 < b.info["n_flipped_rows"] < o.info["n_flipped_rows"] and b.key_order.tobytes() == o.key_order.tobytes()


# ---- the model against the oracle's own commands ----
def test_text_cases_hold_what_they_are_named_for():
    c = pr.orient_text_cases()[0]
    m = pr.model(c)
    key = {(t, q): int(k) for t, q, k in zip(c.t_name, c.q_name, c.rec_key)}
    assert m.key_flip[key["T1", "qa"]] == 1 and m.key_flip[key["T1", "qb"]] == 0 and m.key_flip[key["T0", "qa"]] == 0, "a flipped and an unflipped pair"
    assert int(m.orient[key["T1", "qz"]]) == 0 and m.key_flip[key["T1", "qz"]] == 0, "a key with sum exactly 0"
    assert m.key_order[key["T0", "qc"]] == m.key_order[key["T0", "qd"]], "a scaffold tie"
    names = [ln.split(b"\t")[0] for ln in pr.lines_of(c, m, scaffold=True).splitlines()]
    assert names[0] == b"qc+::qd+::qa+" and c.t_name.index("T0") > c.t_name.index("T1"), "T0 sorts first and appears second"
    order = sorted(range(len(c.t_st)), key=lambda r: (c.t_name[r], int(m.key_order[c.rec_key[r]]), int(m.q_st[r])))
    assert [c.q_name[r] for r in order[:4]] == ["qc", "qd", "qc", "qd"], "... that interleaves two query names"
    for c in pr.filter_text_cases():
        m = pr.model(c)
        if c.name == "filter --paired-len 114":
            assert not m.keep[:3].any() and m.keep[-2:].all() and int(m.fspan[key["T1", "qa"]]) == 114
        if c.name == "filter --paired-len 113":
            assert m.keep[:3].all()
        if c.name == "filter -p 81 -a 33 -q 100":
            assert m.passes[[0, 2]].all() and not m.passes[1] and not m.keep[:3].any(), "a kept ... "
        if c.name == "filter -p 80 -a 33 -q 100":
            assert m.keep[[0, 2]].all() and not m.keep[1], "... and a dropped record of one key"
            assert not m.keep[c.q_name.index("qshort")] and m.keep[c.q_name.index("qlong")]


@pytest.mark.parametrize("c", pr.orient_text_cases(), ids=lambda c: c.name)
def test_model_is_the_oracles_orient(oracle, tmp_path, c):
    paf = tmp_path / "in.paf"
    paf.write_bytes(pr.paf_text(c))
    m = pr.model(c)
    assert m.info["declined"] == 0
    assert oracle.cli("orient", str(paf)) == (0, pr.lines_of(c, m))
    assert oracle.cli("orient", "--scaffold", "--insert", c.insert, str(paf)) == (0, pr.lines_of(c, m, scaffold=True))


@pytest.mark.parametrize("c", pr.filter_text_cases(), ids=lambda c: c.name)
def test_model_is_the_oracles_filter(oracle, tmp_path, c):
    paf = tmp_path / "in.paf"
    paf.write_bytes(pr.paf_text(c))
    m = pr.model(c)
    want = pr.lines_of(c, m)
    assert oracle.cli("filter", *pr.filter_flags(c), str(paf)) == (0, want)
    assert want.count(b"\n") == len(m.kept) and (c.name == "filter defaults") == (len(m.kept) == len(c.t_st))
