"""No GPU: the plain-Python model of tests/nftext_util.py prints what the oracle prints, its decimals are Python's, and the hand-made
cases of tests/test_gpu_nucfreq_text.py contain what that file says they do."""
import itertools

import numpy as np
import pytest

import nf_util
import nftext_util as nu

S, W = 64, 1024  # rb_nucfreq_text_shape() of the shipped kernel (the GPU file asserts S and takes W from the library)


# the regions as the front end cuts them: -r regions and BED rows with ids, one longer than a print piece of 1 Mbp
BAMS = {
    "asm_small.bam": [("chr22", 9000000, 10060000, "long"), ("chr21", 8933000, 8936000, "a"), ("chr22", 10024300, 10024400, "b"), ("chr22", 10030000, 10031000, "c")],
    "test_nucfreq.bam": [("CHROMOSOME_I", 0, 200, "x"), ("CHROMOSOME_II", 5, 50, "none")],
}


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("bam", sorted(BAMS))
def test_model_prints_what_the_oracle_prints(oracle, golden, tmp_path, bam, small):
    names, lens, rd = nf_util.read_bam(f"{golden}/{bam}")
    regions = BAMS[bam]
    bed = tmp_path / "r.bed"
    bed.write_text("".join(f"{n}\t{a}\t{b}\t{i}\n" for n, a, b, i in regions))
    rc, want = oracle.cli("nucfreq", *(["-s"] if small else []), "--bed", bed, f"{golden}/{bam}")
    assert rc == 0
    got, n_lines, longest = nu.oracle_text(oracle, rd.args(), names, lens, regions, small)
    assert got == want
    if bam == "asm_small.bam":
        assert n_lines >= 1000 and longest > nu.MED
    else:
        assert n_lines >= 50


def test_decimals_are_pythons():
    vals = set(nu.CGT_SEAMS) | {p + d for p in nu.POS_SEAMS for d in (0, 1, 2)} | {10 ** k for k in range(11)} | {(1 << 32) - 1, (1 << 64) - 1}
    vals |= set(np.random.default_rng(1).integers(0, 1 << 32, 2000).tolist())
    for v in vals:
        assert nu.dec(v) == str(v).encode()
    assert nu.full_line(b"c\t", (1 << 32) - 1, 1, 2, 3, 4, b"\ti\n") == b"c\t4294967295\t0\t1\t2\t3\t4\ti\n"
    assert nu.small_line(3, 9, 9, 1) == b"9\t9\n" and nu.small_line(0, 0, 7, 0) == b"7\t0\n"


def _fields(case):
    """(position, A, C, G, T) of every line of a case"""
    out = []
    for s in range(len(case.seg_n)):
        c0, p0 = int(case.seg_cnt[s]), int(case.seg_pos[s])
        for k in range(int(case.seg_n[s])):
            r = [int(x) for x in case.counts[c0 + k]]
            if r[0] & nu.COVERED:
                out.append((p0 + k, r[0] & (nu.COVERED - 1), r[1], r[2], r[3]))
    return out


def test_digit_seams_hold_every_digit_count():
    f = _fields(nu.digit_seams(nu.FULL))
    for col, most in ((0, 10), (1, 10), (2, 10), (3, 10), (4, 10)):
        assert {len(str(r[col])) for r in f} == set(range(1, most + 1)), col
    a = {r[1] for r in f}
    assert {0, 9, 10, 65535, (1 << 31) - 1} <= a and max(a) == (1 << 31) - 1
    for col in (2, 3, 4):
        assert {0, 9, 10, 65535, (1 << 32) - 1} <= {r[col] for r in f}
    pos = {r[0] for r in f}
    for k in range(1, 10):
        assert {10 ** k - 1, 10 ** k} <= pos
    assert {(1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1} <= pos
    text = nu.model(nu.digit_seams(nu.FULL))[0]
    assert b"chrP\t4294967295\t0\t" in text and b"chrP\t4294967294\t4294967295\t" in text


def test_phases_hold_every_phase_and_length():
    for mode in (nu.FULL, nu.SMALL):
        c = nu.phases(mode)
        text, off, _, lines, starts = nu.model(c)
        assert {s % 16 for s in starts} == set(range(16))
    c = nu.phases(nu.FULL)
    assert {(len(a), len(b)) for a, b in zip(c.pre, c.suf)} == set(itertools.product([0, 1, 15, 16, 17, 255], repeat=2))
    assert (c.seg_n > S).all()
    # the longest lines: one step of them is more than the 4096 bytes the print kernel stages at a time
    k = [i for i, (a, b) in enumerate(zip(c.pre, c.suf)) if len(a) == 255 and len(b) == 255][0]
    off = nu.model(c)[1]
    assert int(off[k + 1] - off[k]) * S // int(c.seg_n[k]) > 4096


def test_run_lengths_and_coverage_patterns():
    assert {0, 1, S - 1, S, S + 1, W - 1, W, W + 1, 2 * W + 1} <= set(nu.run_length_list(S, W))
    c = nu.run_lengths(nu.FULL, S, W)
    assert sorted(c.seg_n.tolist()) == nu.run_length_list(S, W)
    c = nu.coverage(nu.FULL, S, W)
    _, off, first, lines, _ = nu.model(c)
    cov0 = (c.counts[int(c.seg_cnt[0]):int(c.seg_cnt[0]) + int(c.seg_n[0]), 0] & nu.COVERED) != 0
    gaps = [len(list(g)) for v, g in itertools.groupby(cov0.tolist()) if not v]
    assert any(2 * S <= g < W for g in gaps) and any(g >= 2 * W for g in gaps)  # a whole step / a whole workgroup wherever they are cut
    n = int(c.seg_n[1])
    assert int(lines[1]) == 1 and int(first[1]) == int(c.seg_pos[1])
    assert int(lines[2]) == 1 and int(first[2]) == int(c.seg_pos[2]) + n - 1
    for s in (3, 4, 5):
        assert int(lines[s]) == 0 and int(first[s]) == nu.NONE and off[s] == off[s + 1]
    assert (c.counts[:, 1:] != 0).any(axis=1).all()  # (uncovered positions hold counts too: only the bit decides)


def test_many_short_overlapping_and_shuffled():
    c = nu.many_short(nu.FULL)
    _, off, _, lines, _ = nu.model(c)
    assert len(c.seg_n) == 3000 and set(c.seg_n.tolist()) == {1, 2, 3, 4, 5}
    assert {int(o) % 16 for o in off} == set(range(16)) and (lines == 0).any()
    c = nu.overlapping(nu.FULL)
    iv = [(int(a), int(a) + int(n)) for a, n in zip(c.seg_cnt, c.seg_n)]
    assert any(a < d and c_ < b for (a, b), (c_, d) in itertools.combinations(iv, 2))
    assert iv[1] == iv[2] and iv[0][0] <= iv[1][0] and iv[1][1] <= iv[0][1]
    c = nu.shuffled_layout(nu.FULL)
    nz = c.seg_cnt[c.seg_n > 0]
    assert not np.array_equal(nz, np.sort(nz)) and (c.seg_n == 0).any()


def test_small_orders():
    c = nu.small_orders()
    rows = [[int(x) for x in r] for r in c.counts]
    perms = {tuple(r[0] & (nu.COVERED - 1) if i == 0 else r[i] for i in range(4)) for r in rows[:24]}
    assert perms == set(itertools.permutations([3, 45, 678, 9012]))
    vals = [(r[0] & (nu.COVERED - 1), r[1], r[2], r[3]) for r in rows if r[0] & nu.COVERED]
    srt = [sorted(v) for v in vals]
    assert any(v[3] == v[2] != v[1] for v in srt) and any(v[3] != v[2] == v[1] for v in srt) and any(v[0] == v[3] for v in srt)
    assert any(v[0] == 0 and max(v) > 0 for v in vals) and any(v[0] == max(v) and v[0] > v[1] for v in vals)
    text = nu.model(c)[0]
    assert text.count(b"\n") == len(vals) == len(rows) - 1
    assert b"2147483648" not in text.split(b"\n")[0]  # (the covered bit is not part of A)
    assert text.startswith(b"9012\t678\n")


def test_every_case_name_builds():
    for name in nu.CASE_NAMES:
        c = nu.get_case(name, S, W)
        text, off, first, lines, starts = nu.model(c)
        assert int(off[-1]) == len(text) and len(starts) == int(lines.sum())
        if name != "small_orders":
            assert int(lines.sum()) > 50
