"""The inputs and the model of the rb_dev_bam_reads tests (tests/bam_reads_util.py) hold what they claim: the case generators cover every
phase, seam and count the GPU file relies on, the fast twin for uniform files equals the plain model, and the model's end_key_pmax and
start_key give slices that hold every read the oracle's nucfreq counts.  No GPU here."""
import numpy as np
import pytest

import bam_rec_util as B
import bam_reads_util as R
import nf_util as N

SHAPES = [(64, 4096, 256, 512), (64, 1024, 256, 128)]  # the shipped shape and one a variant build could have


def _model_of(cases):
    data, off, ln = B.stream([b for _, b in cases])
    m = B.model(data, off, ln)
    return (data, off, ln), m, R.model(data, off, ln, m)


def test_seq_cases_cover_every_phase_and_refusal():
    cases = R.seq_cases()
    (data, off, ln), m, md = _model_of(cases)
    labels = [lb for lb, _ in cases]
    ok = m["status"] == B.BAM_OK
    assert {int(x) % 16 for x in md["seq_off"][ok]} == set(range(16))
    assert (md["seq_off"][~ok] == 0).all() and sorted(set(m["status"].tolist())) == [0, 1, 2, 3]
    k = labels.index("cg_70000")
    assert int(m["op_off"][k + 1] - m["op_off"][k]) == 70000
    assert int(md["seq_off"][k]) == int(off[k]) + 32 + 3 + 8  # behind the two in-record words, not behind the tag's
    assert data[int(md["seq_off"][k]):int(md["seq_off"][k]) + 3] == b"\xff" * 3
    ls = {lb: int(m["l_seq"][i]) for i, lb in enumerate(labels)}
    assert ls["l_seq_0"] == 0 and ls["l_seq_odd"] % 2 == 1
    for i in np.flatnonzero(ok):  # the model's seq_off is where body() put the bases
        a = int(md["seq_off"][i])
        n = (int(m["l_seq"][i]) + 1) // 2
        assert data[a:a + n] == b"\xff" * n and a + n <= int(off[i]) + int(ln[i])


@pytest.mark.parametrize("shape", SHAPES)
def test_ref_cases_cover_every_seam_and_a_sum_behind_32_bits(shape):
    cases = R.ref_cases(shape)
    _, m, md = _model_of(cases)
    labels = [lb for lb, _ in cases]
    n_ops = np.diff(m["op_off"]).astype(np.int64)
    want = {0, 1, 15, 16, 17} | {v + d for v in shape for d in (-1, 0, 1)}
    for nc in want:  # every count at every dword phase of the first op
        ph = {int(m["op_off"][i]) % 4 for i, lb in enumerate(labels) if lb.startswith(f"ops_{nc}_")}
        assert ph == {0, 1, 2, 3}, (nc, ph)
        assert all(n_ops[labels.index(f"ops_{nc}_{k}")] == nc for k in range(4))
    ref = dict(zip(labels, md["ref"]))
    assert ref["only_I_S_H_P"] == 0 and ref["sum_behind_2^32"] == 20 * (2**28 - 1) > 2**32
    ek = dict(zip(labels, (int(x) for x in md["end_key_pmax"])))
    assert ek["sum_behind_2^32"] & 0xFFFFFFFF == 0xFFFFFFFF
    k = labels.index("only_I_S_H_P")
    assert int(md["end_key_pmax"][k]) == max(int(md["end_key_pmax"][k - 1]), R.nf_key(0, 5000 + 1))
    k = labels.index("every_nibble")
    assert sorted(int(x) & 15 for x in m["ops"][int(m["op_off"][k]):int(m["op_off"][k + 1])]) == list(range(16))
    assert ref["every_nibble"] == sum(k + 2 for k in (0, 2, 3, 7, 8))
    assert ref["endpos_2^32"] + 2**31 - 1 == 2**32 and ref["endpos_2^32-1"] + 2**31 - 1 == 2**32 - 1
    assert R.nf_key(0, -5) == 0xFFFFFFFF and R.nf_key(-1, 7) == (0xFFFFFFFF << 32) | 7 and R.nf_key(3, 2**32) == (3 << 32) | 0xFFFFFFFF


def test_enters_cases_say_who_enters():
    cases = R.enters_cases()
    _, m, md = _model_of(cases)
    labels = [lb for lb, _ in cases]
    e = dict(zip(labels, md["enters"].tolist()))
    assert not any(e[f"flag_{b:#x}_alone"] for b in (0x4, 0x100, 0x200, 0x400)) and all(e[f"behind_flag_{b:#x}"] for b in (0x4, 0x100, 0x200, 0x400))
    assert all(e[f"flag_{b:#x}_enters"] for b in (0x1, 0x2, 0x8, 0x10, 0x20, 0x40, 0x80, 0x800))
    assert not e["tid_-1"] and e["pos_-1_tid_0"] and not e["refused"] and not e["unmapped_with_a_cigar"]
    assert m["status"][labels.index("refused")] == B.BAM_BAD_NAME
    pm = md["end_key_pmax"]
    for i, lb in enumerate(labels):  # a read that does not enter carries the value in front of it, though its own end would be the largest
        if not e[lb]:
            assert int(pm[i]) == (int(pm[i - 1]) if i else 0), lb
    k = labels.index("pos_-1_tid_0")
    assert int(pm[k]) == R.nf_key(0, 300000) and int(md["start_key"][k]) == 0xFFFFFFFF  # endpos from max(pos, 0); the start key saturates
    k = labels.index("no_ops_reaches_pos_plus_1")
    assert int(pm[k]) == R.nf_key(1, 2**30 + 6)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_uniform_twin_equals_the_plain_model(shape):
    blk = shape[3]
    files = [R.scan_file(n, blk) for n in (0, 1, 65, blk + 1, 3 * blk + 7)] + [u for u, _ in R.unsorted_files().values()]
    u = R.scan_file(200, blk)
    u["flag"][::7] |= 4          # (unmapped records: no ops, their end is pos + 1 and they do not enter)
    u["pos"][5], u["tid"][190:] = -1, -1
    u["opc"] = np.arange(200) % 16
    files.append(u)
    for u in files:
        data, off, ln = R.uniform_stream(u)
        assert B.hop(data)[1].tolist() == off.tolist() and B.hop(data)[2].tolist() == ln.tolist()
        m = B.model(data, off, ln)
        md = R.model(data, off, ln, m)
        fast = R.uniform_model(u, off)
        for k in B.COLS + ("op_off", "ops"):
            assert np.array_equal(fast[k], m[k]), k
        for k in R.OUTS + ("first_unsorted", "enters"):
            assert np.array_equal(fast[k], md[k]), k


@pytest.mark.parametrize("shape", SHAPES)
def test_scan_files_put_the_carries_to_work(shape):
    blk = shape[3]
    counts = R.scan_counts(blk)
    assert {0, 1, 63, 64, 65, blk - 1, blk, blk + 1, blk * blk + 1} <= set(counts)
    n = blk * blk + 1
    u = R.scan_file(n, blk)
    data_off = np.zeros(n, np.uint64)
    f = R.uniform_model(u, data_off)
    assert int(f["first_unsorted"][0]) == R.NONE and sorted(set(u["tid"].tolist())) == [0, 1, 2]
    pm = f["end_key_pmax"][:blk * blk].reshape(blk, blk)
    same_tid = u["tid"][:blk * blk].reshape(blk, blk)
    same_tid = same_tid[:, 0] == same_tid[:, -1]
    even, odd = np.arange(blk) % 2 == 0, (np.arange(blk) % 2 == 1) & (np.arange(blk) < blk - 1)  # (the last one ends in reads that do not enter)
    # even workgroups: the first record's end is the workgroup's maximum; odd ones: the last record raises it
    assert (pm[even & same_tid, 0] == pm[even & same_tid, -1]).all() and (pm[odd, -2] < pm[odd, -1]).all() and (even & same_tid).sum() > blk // 4
    e = f["enters"]
    for seam in (blk, 3 * blk, blk * blk):  # a run of reads that do not enter lies across the seam
        assert not e[seam - 2:seam + 2].any() and f["end_key_pmax"][seam - 2] == f["end_key_pmax"][min(seam + 1, n - 1)]
    steps = np.flatnonzero(np.diff(u["tid"])) + 1
    assert len(steps) == 2 and all(int(f["end_key_pmax"][s]) >> 32 == int(u["tid"][s]) for s in steps if e[s])


def test_unsorted_files_say_where():
    files = R.unsorted_files()
    assert {"none", "at_1", "at_n-1", "two_candidates_the_smaller_wins", "masked_by_tid", "masked_by_pos"} <= set(files)
    for lb, (u, want) in files.items():
        data, off, ln = R.uniform_stream(u)
        md = R.model(data, off, ln)
        assert int(md["first_unsorted"][0]) == want, lb
        sk = md["start_key"].astype(object)
        n_back = sum(1 for i in range(1, len(sk)) if sk[i] < sk[i - 1])
        assert n_back == (0 if lb == "none" else 2 if lb.startswith("two") else 1), lb  # (the masked files do step back: that is what is masked)
    u, _ = files["two_candidates_the_smaller_wins"]
    back = [i for i in range(1, 300) if u["pos"][i] < u["pos"][i - 1]]
    assert back == [70, 200] and back[0] // 16 != back[1] // 16  # (16 records to a workgroup of the per-record pass, 4 to a wavefront)


@pytest.mark.parametrize("seed", [1, 2])
def test_slices_from_the_model_hold_every_read_the_oracle_counts(oracle, seed):
    """nucfreq_bam's slice [i0, i1) from end_key_pmax and start_key: no read outside it overlaps the positions, and the oracle's pileup of
    the slice is its pileup of the whole file"""
    rng = np.random.default_rng(seed)
    reads = N.random_reads(rng, 400, n_contig=2, span=6000, max_ops=12)
    data, off, ln = R.reads_stream(reads)
    m = B.model(data, off, ln)
    md = R.model(data, off, ln, m)
    n = reads.n
    assert (m["status"] == 0).all() and len(off) == n + 1 and int(md["first_unsorted"][0]) == R.NONE
    assert np.array_equal(m["tid"][:n], reads.tid) and np.array_equal(m["pos"][:n], reads.pos)
    assert {int(x) % 16 for x in md["seq_off"][:n]} == set(range(16))
    for i in (0, 7, n - 1):  # the model's seq_off is where the bases are
        a, k = int(md["seq_off"][i]), (int(reads.l_seq[i]) + 1) // 2
        assert data[a:a + k] == reads.seq[int(reads.seq_off[i]):int(reads.seq_off[i]) + k].tobytes()
    end = np.array([int(reads.pos[i]) + max(md["ref"][i], 1) for i in range(n)])
    n_checked = 0
    for _ in range(30):
        tid = int(rng.integers(0, 2))
        st = int(rng.integers(0, 9000))
        en = st + int(rng.integers(1, 3000))
        i0, i1 = R.slice_of(md, tid, st, en)
        assert 0 <= i0 <= i1 <= n + 1
        hit = np.flatnonzero(md["enters"][:n] & (reads.tid == tid) & (reads.pos < en) & (end > st))
        assert all(i0 <= i < i1 for i in hit), (tid, st, en, i0, i1, hit[:5])
        whole = oracle.nucfreq(*reads.args(), tid, st, en)
        part = oracle.nucfreq(*reads.slice(i0, min(i1, n)).args(), tid, st, en)
        assert whole[0] == part[0] == 0 and np.array_equal(whole[1], part[1]) and np.array_equal(whole[2], part[2])
        n_checked += len(whole[1]) > 0 and (i0 > 0 or i1 < n)
    assert n_checked >= 10  # (real slices of covered regions, not the whole file each time)


def test_the_three_islands_lie_in_members_far_apart():
    """the file of the index-range test: every group's records in a run of BGZF members with dozens of untouched members in between, and a
    record of the first group that straddles two members for the index to end in"""
    refs, recs, bed = R.three_islands()
    raw, bai, start = R.bgzf_and_bai(refs, recs)
    assert raw.count(b"\x1f\x8b\x08\x04") >= start[-1] // 512 and bai[:4] == b"BAI\x01"
    members = {g: {u // 512 for r, rec in enumerate(recs) if rec["name"].startswith(g) for u in (start[r], start[r + 1] - 1)} for g in "abc"}
    assert max(members["a"]) + 20 < min(members["b"]) and max(members["b"]) + 15 < min(members["c"])
    assert any((start[r] + 10) // 512 < (start[r + 1] - 1) // 512 for r in range(10, 30))
    assert len({l.split("\t")[0] for l in bed.splitlines()}) == 2 and [l.split("\t")[0] for l in bed.splitlines()][:2] == ["chrB", "chrA"]
    cut = R.bgzf_and_bai(refs, recs, cut_in=12)[1]
    assert cut != bai and len(cut) == len(bai)
