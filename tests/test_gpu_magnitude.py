"""The clip and pair kernels where 32 bits run out (tests/magnitude_util.py builds the inputs, tests/test_magnitude_inputs.py proves what they
hold and pins the references on the CPU).

1. Coordinates at and past 2^32: the batches of the other test files SHIFTED far out, still against the per-base oracle (it keeps positions
   in u64 and costs memory per aligned unit, not per coordinate).  The fast kernels work in 32-bit offsets from a record's start; a
   dropped high half, a start and an end on different sides of 2^32, or an offset taken from 0 instead shows here.
2. Regular records of 2^31 .. 2^32 - 1 units, at the thresholds the fast kernels guard their 32-bit prefixes with, against clip_regular /
   break_regular (run-length form, exact integers).
3. The pair row kernel's score guard (k_trim4.hip: smax * (Lq + Rq) >= 2^29 leaves it to the wave-per-pair kernel, which sums in 64 bits).

Every test states its route: n_generic (the stream kernel did it), phase[3] / phase[4] (tiles made / records handed back), the pair row's
diagnostic word (_row 1: the row kernel; _pad 1 and _row 0: the wave-per-pair kernel; both 0: the serial kernel)."""
import os
import subprocess

import numpy as np
import pytest

import magnitude_util as mu
import rustybam_amd
from rustybam_amd import trim_driver
from devutil import DevBatch
from rbtest_util import batch_args, compare_hits, digest_rows, random_batch, random_windows, recs_from_lines
from test_gpu_parity import _check_liftover, _obatch, _rebuild_from_descriptor
from test_gpu_tile import FUSED, break_both, lift_both, sliding, synth_batch, tile_env
from test_gpu_trim import _compare, _pairs_batch
from test_magnitude_inputs import TILE_CASES, lane_case, spans_case, tile_case
from trim_util import format_resident

pytestmark = pytest.mark.gpu
MODERN, LEGACY = rustybam_amd.BSEARCH_MODERN, rustybam_amd.BSEARCH_LEGACY
ONE_WALK = rustybam_amd.BREAK_ONE_WALK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = os.path.join(ROOT, "rustybam_amd", "rb")
SHIFT_IDS = ["straddle_2p32", "past_2p32", "2p40_2p52", "2p62"]
shifts = pytest.mark.parametrize("K", mu.SHIFTS, ids=SHIFT_IDS)


def _moved(rows, K, what):
    """rows of the unshifted call, as the shifted call must return them"""
    want = rows.copy()
    ok = want["status"] == 0
    for k, d in (("t_st", K[0]), ("t_en", K[0]), ("q_st", K[1]), ("q_en", K[1])):
        want[k][ok] += np.uint64(d)
    return want


def _same_but_moved(rows, ops, rows0, ops0, K, what):
    """shifting is a bijection on the records: the shifted call returns the unshifted call's rows, moved, and the same clips"""
    want = _moved(rows0, K, what)
    assert len(rows) == len(want), what
    for k in ("rec", "win", "status", "out_n", "t_st", "t_en", "q_st", "q_en", "nmatch", "aln_len"):
        sel = want["status"] == 0 if k not in ("rec", "win", "status") else slice(None)
        assert np.array_equal(rows[k][sel], want[k][sel]), f"{what}: {k} is not the unshifted call's, moved"
    for g, o in zip(rows, rows0):
        if o["status"] == 0:
            assert np.array_equal(ops[int(g["out_off"]):int(g["out_off"]) + int(g["out_n"])], ops0[int(o["out_off"]):int(o["out_off"]) + int(o["out_n"])]), what


# ================================================================== 1. shifted batches against the per-base oracle
@shifts
@pytest.mark.parametrize("policy", [MODERN, LEGACY])
def test_liftover_shifted(engine, oracle, K, policy):
    """stand-alone scan, fused scan and the oracle (_check_liftover) on 300 records under 120 windows moved by K"""
    import zlib
    for mode, monotone in (("regular", True), ("regular", False), ("indel_ends", True), ("mixed", False), ("spliced", True)):
        rng = np.random.default_rng(zlib.crc32(f"mag{mode}{monotone}".encode()))
        b0 = random_batch(rng, 300, mode, n_contig=3)
        w0 = random_windows(rng, b0, 120, monotone)
        b, w = mu.shift(b0, w0, *K)
        what = f"{mode} mono={monotone} K={K}"
        rows, cnt = _check_liftover(engine, oracle, b, w, policy, what)
        assert len(rows) > 100
        if mode == "regular":
            # the streaming kernel did every clip (the legacy policy sends the clips whose boundary falls on an insertion's base to the
            # generic kernel, which replays the old binary search: a few, and as many as below 2^32)
            assert cnt["n_generic"] == 0 or policy == LEGACY, what
            rows0, ops0, _, _ = engine.liftover(*batch_args(b0), b0["contig"], *w0, policy=policy)
            rows1, ops1, _, _ = engine.liftover(*batch_args(b), b["contig"], *w, policy=policy)
            _same_but_moved(rows1, ops1, rows0, ops0, K, what)
        if mode == "spliced":
            assert cnt["n_generic"] < len(rows) // 4, what


@shifts
def test_liftover_shifted_many_passes_and_minus_strand(engine, oracle, K):
    """more than 64 windows per record (several streaming passes over one record, the offsets carried from pass to pass), and records on
    the '-' strand only (q_en - Q: the subtraction from a query end past 2^32)"""
    rng = np.random.default_rng(11)
    b0 = random_batch(rng, 40, "regular", n_contig=1, long_frac=1.0)
    st = np.arange(0, int(b0["t_en"].max()), 37, dtype=np.uint64)
    b, w = mu.shift(b0, (np.zeros(len(st), np.uint32), st, st + np.uint64(50)), *K)
    rows, cnt = _check_liftover(engine, oracle, b, w, MODERN, f"dense windows K={K}")
    assert len(rows) > 64 * 40 and cnt["n_generic"] == 0
    b0 = random_batch(rng, 300, "regular", n_contig=2)
    b0["strand"][:] = ord("-")
    b, w = mu.shift(b0, random_windows(rng, b0, 120, True), *K)
    for policy in (MODERN, LEGACY):
        rows, cnt = _check_liftover(engine, oracle, b, w, policy, f"minus strand K={K}")
        assert len(rows) > 100 and (cnt["n_generic"] == 0 or policy == LEGACY)


@shifts
@pytest.mark.parametrize("lo,hi,n", [(8, 130, 900), (300, 700, 600)])
def test_tile_kernel_shifted(engine, oracle, K, lo, hi, n):
    """the generator and the comparisons of tests/test_gpu_tile.py (tiles == per record == oracle), moved by K: the tile kernel keeps one
    running total across all records of a tile and adds it to each record's own start"""
    b0 = synth_batch(engine, 0x7117 + lo, n, lo, hi, span=400_000)
    b, w = mu.shift(b0, sliding(span=600_000, step=41_398, width=50_000), *K)
    for policy in (FUSED, FUSED | LEGACY):
        cnt = lift_both(engine, oracle, b, w, policy, f"tiles {lo}-{hi} K={K} policy {policy}")
        assert int(cnt["phase"][3]) > 0, "no tiles were made"
    for max_size in (0, 100):
        for policy in (FUSED, FUSED | ONE_WALK):
            cnt = break_both(engine, oracle, b, max_size, policy, f"tiles {lo}-{hi} K={K} break {max_size} policy {policy}")
            assert int(cnt["phase"][3]) > 0, "no tiles were made"


@shifts
@pytest.mark.parametrize("policy", [MODERN, LEGACY])
def test_break_paf_shifted(engine, oracle, K, policy):
    for max_size in (0, 2, 100):
        rng = np.random.default_rng(5 + max_size)
        for mode in ("mixed", "regular"):
            b0 = random_batch(rng, 300, mode)
            b, _ = mu.shift(b0, None, *K)
            what = f"break {mode} max={max_size} K={K}"
            orows, oops = oracle.break_paf(_obatch(oracle, b), max_size, policy=policy)
            rows, ops, norm, cnt = engine.break_paf(*batch_args(b), max_size, policy=policy)
            compare_hits(rows, ops, orows, oops, what)
            for extra in (rustybam_amd.LIFT_FUSED_SCAN, rustybam_amd.LIFT_FUSED_SCAN | ONE_WALK, ONE_WALK):
                frows, fops, fnorm, _ = engine.break_paf(*batch_args(b), max_size, policy=policy | extra)
                assert np.array_equal(fnorm["status"], norm["status"]) and not (fnorm["flags"] & 8).any()
                keep = (norm["status"] == 0)[frows["rec"]] if len(frows) else np.zeros(0, bool)
                compare_hits(frows[keep], fops, orows, oops, f"{what} policy {policy | extra}")
            if mode == "regular":
                assert cnt["n_generic"] == 0 or policy == LEGACY, what
                rows0, ops0, _, _ = engine.break_paf(*batch_args(b0), max_size, policy=policy)
                _same_but_moved(rows, ops, rows0, ops0, K, what)


def test_descriptors_and_early_exit_shifted(engine, oracle):
    """RB_LIFT_DESCRIPTORS / RB_LIFT_EARLY_EXIT describe the clips of the default mode, past 2^32 as below it"""
    rng = np.random.default_rng(77)
    b0 = random_batch(rng, 400, "regular", n_contig=2, long_frac=0.3)
    b, w = mu.shift(b0, random_windows(rng, b0, 150, True), *mu.SHIFTS[1])
    base_rows, base_ops, _, cnt = engine.liftover(*batch_args(b), b["contig"], *w)
    orows, oops = oracle.liftover(_obatch(oracle, b), *w)
    compare_hits(base_rows, base_ops, orows, oops, "default mode")
    assert cnt["n_generic"] == 0
    for pol in (rustybam_amd.LIFT_EARLY_EXIT, rustybam_amd.LIFT_DESCRIPTORS, rustybam_amd.LIFT_DESCRIPTORS | rustybam_amd.LIFT_EARLY_EXIT):
        rows, ops, _, cnt = engine.liftover(*batch_args(b), b["contig"], *w, policy=pol)
        assert len(rows) == len(base_rows) and cnt["n_generic"] == 0
        for k in ("rec", "win", "status", "t_st", "t_en", "q_st", "q_en", "nmatch", "aln_len", "out_n"):
            assert np.array_equal(rows[k], base_rows[k]), (pol, k)
        n_desc = 0
        for g, o in zip(rows, base_rows):
            if int(o["status"]) != 0:
                continue
            want = base_ops[int(o["out_off"]):int(o["out_off"]) + int(o["out_n"])]
            if int(g["flags"]) & rustybam_amd.HIT_DESCRIPTOR:
                got = _rebuild_from_descriptor(b, g, ops[int(g["out_off"]):int(g["out_off"]) + 4])
                n_desc += 1
            else:
                got = ops[int(g["out_off"]):int(g["out_off"]) + int(g["out_n"])]
            assert np.array_equal(got, want), (pol, int(g["rec"]), int(g["win"]))
        if pol & rustybam_amd.LIFT_DESCRIPTORS:
            assert n_desc == int((base_rows["status"] == 0).sum())


def _shift_pairs(b, K):
    return mu.shift(b, None, *K)[0]


@shifts
@pytest.mark.parametrize("policy", [MODERN, LEGACY])
def test_pairs_shifted(engine, oracle, K, policy):
    """_pairs_batch moved by K: short records (the row kernel's) and records of 600 .. 900 ops with overlaps of any width (which leave the
    row kernel's regions for the wave-per-pair kernel); both must have taken some"""
    by_row = by_wave = 0
    for seed, ops_range, n_pairs in ((1, (3, 60), 200), (2, (600, 900), 30)):
        rng = np.random.default_rng(7100 + seed)
        b0, left, right = _pairs_batch(rng, n_pairs, "regular", ops_range=ops_range)
        b = _shift_pairs(b0, K)
        ob = oracle.Batch(*batch_args(b))
        for scores in ((1, 1, 1), (3, 1, 7)):
            rows, out = engine.overlap_split(*batch_args(b), left, right, scores, policy)
            orows, oout = oracle.overlap_split(ob, left, right, scores, policy)
            _compare(rows, out, orows, oout, f"pairs {ops_range} {scores} K={K} policy {policy}")
            assert (orows["status"] == 0).sum() > n_pairs // 2
            by_row += int((rows["_row"] == 1).sum())
            by_wave += int(((rows["_pad"] == 1) & (rows["_row"] == 0)).sum())
    assert by_row > 0 and by_wave > 0, (by_row, by_wave)


@shifts
@pytest.mark.parametrize("cfg", ["default", "legacy"])
def test_resident_trim_shifted(oracle, tmp_path, K, cfg):
    """RB_TRIM_IN_PLACE through trim_driver.ResidentTrim on 2,000 shifted regular records of 40 .. 120 ops, four to a query: every pair is
    cut where it lies, and the gathered batch prints as the oracle CLI prints the file"""
    import torch
    from trim_util import CONFIGS, oracle_args
    text = mu.shift_paf_text(mu.trim_groups_text(7), *K)
    path = tmp_path / "shifted.paf"
    path.write_text(text)
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    r = recs_from_lines(text.splitlines())
    rank = {q: i for i, q in enumerate(sorted(set(r.q_name)))}
    T = trim_driver.ResidentTrim(eng, torch, dev, r.ops, r.op_off, r.t_st, r.t_en, r.q_st, r.q_en, r.strand, np.array([rank[q] for q in r.q_name]))
    norm0 = T.d_norm.cpu().numpy().view(rustybam_amd.NORM_DT)[:r.n].copy()
    T.run(CONFIGS[cfg]["scores"], CONFIGS[cfg]["policy"])
    assert T.passes >= 2 and T.pairs_done >= 1000 and T.pairs_by_wave == T.pairs_done  # (in place: no pair went to the serial kernel)
    d_new, new_off, norm = T.gather()
    got = format_resident(r, norm0, norm, d_new.cpu().numpy().view(np.uint32), new_off, T.order)
    orc, want = oracle.cli(*oracle_args(cfg, str(path)))
    assert orc == 0 and got.encode() == want
    del d_new
    T.release()
    torch.cuda.synchronize()
    eng.close()


@shifts
def test_digest_rows_shifted(oracle, K):
    """rb_dev_digest_rows folds the 64-bit coordinates of every row: equal to its numpy twin on the oracle's rows"""
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(77)
    b0 = random_batch(rng, 300, "regular", n_contig=1, long_frac=0.2)
    b, w = mu.shift(b0, random_windows(rng, b0, 80, True), *K)
    orows, oops = oracle.liftover(_obatch(oracle, b), *w)
    want = digest_rows(orows, oops)
    D = DevBatch(torch, eng, dev, b)
    rows, out, cnt = D.run(w)
    assert rows.shape[0] == len(orows) and len(orows) > 100 and cnt["n_generic"] == 0
    assert D.digest(rows, out) == want
    moved = orows.copy()
    moved["q_en"][0] ^= np.uint64(1 << 32)  # (a bit of a high half changes it)
    assert digest_rows(moved, oops) != want
    eng.close()


# ---- the front end
FRONT_K = 2**32 + 12345
COMMANDS = {
    "liftover": ["liftover", "--bed", "{bed}", "{paf}"],
    "liftover_legacy": ["--bsearch", "legacy", "liftover", "--bed", "{bed}", "{paf}"],
    "liftover_largest": ["liftover", "--largest", "--bed", "{bed}", "{paf}"],
    "break_paf": ["break-paf", "--max-size", "100", "{paf}"],
    "trim_paf": ["trim-paf", "{paf}"],
    "invert": ["invert", "{paf}"],
    "stats": ["stats", "--paf", "{paf}"],
}


@pytest.fixture(scope="module")
def shifted_files(golden, tmp_path_factory):
    d = tmp_path_factory.mktemp("shifted")
    paf, bed = d / "asm_small.paf", d / "asm_small.bed"
    paf.write_text(mu.shift_paf_text(open(os.path.join(golden, "asm_small.paf")).read(), FRONT_K, FRONT_K))
    bed.write_text(mu.shift_bed_text(open(os.path.join(golden, "asm_small.bed")).read(), FRONT_K))
    return str(paf), str(bed)


def _move_output(out):
    """what a command printed for the fixture, as it must print it for the shifted fixture: PAF lines and the lines of `stats` hold their
    coordinates and lengths in the same columns (2-4 and 7-9); header lines stay"""
    lines = out.decode().splitlines()
    return "".join(ln + "\n" if ln.startswith("#") else mu.shift_paf_text(ln, FRONT_K, FRONT_K) for ln in lines).encode()


@pytest.mark.parametrize("name", list(COMMANDS))
def test_front_end_on_the_shifted_fixture(oracle, golden, shifted_files, name):
    """`rb` on asm_small.paf moved by 2^32 + 12345 (columns 3, 4, 8, 9, the two lengths, the bed): what the oracle CLI prints, with its
    return code; and the lines `rb` prints for the file where it was, moved"""
    assert os.path.exists(RB), "rustybam_amd/rb missing: run __graft_entry__.build()"
    paf, bed = shifted_files
    run = lambda a: subprocess.run([RB, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE)  # noqa: E731
    args = [x.format(paf=paf, bed=bed) for x in COMMANDS[name]]
    r = run(args)
    orc, want = oracle.cli(*args)
    assert (r.returncode, orc) == (0, 0) and want.count(b"\n") > 3
    assert r.stdout == want
    r0 = run([x.format(paf=os.path.join(golden, "asm_small.paf"), bed=os.path.join(golden, "asm_small.bed")) for x in COMMANDS[name]])
    assert r0.returncode == 0 and _move_output(r0.stdout) == r.stdout


# ================================================================== 2. regular records of 2^31 .. 2^32 - 1 units
def _lift(engine, b, w, policy):
    with tile_env(True):
        return engine.liftover(*batch_args(b), b["contig"], *w, policy=policy)


def _brk(engine, b, max_size, policy):
    with tile_env(True):
        return engine.break_paf(*batch_args(b), max_size, policy=policy)


def _same_norm(fnorm, norm, what):
    assert np.array_equal(fnorm["status"], norm["status"]), f"{what}: fused norm.status"
    for k in ("t_st", "t_en", "q_st", "q_en", "first_op", "n_ops", "nmatch", "aln_len", "lead_ops", "trail_ops"):
        assert np.array_equal(fnorm[k], norm[k]), f"{what}: fused norm.{k}"
    assert not (fnorm["flags"] & 8).any(), f"{what}: a provisional row leaked"


@pytest.mark.parametrize("t_st", [1000, 2**32 - 5])
def test_spans_on_the_stream_kernel(engine, t_st):
    """records of 2^31 - 1, 2^31, 2^31 + 1, 3e9 and 2^32 - 1 units in 15 .. 40 ops, both strands, under windows one base wide at the
    offsets around 2^31 and windows that cut the ops there: the stream kernel's D, Rb / Qb / Ub and its prefix scans at the top of their
    range.  With the stand-alone scan the records are REGULAR and the stream kernel clips them (n_generic == 0); the fused scan returns
    the same rows (its 2^25 lane guard hands such records back: no route asserted)."""
    b, w = spans_case(t_st)
    for policy in (MODERN, LEGACY):
        want = mu.liftover_regular(b, w, policy)
        rows, ops, norm, cnt = _lift(engine, b, w, policy)
        assert (norm["status"] == 0).all() and (norm["flags"] & 1).all(), "the record scan calls these records regular"
        compare_hits(rows, ops, *want, f"spans at {t_st} policy {policy}")
        assert (cnt["n_generic"] == 0 or policy == LEGACY) and (rows["status"] == 0).sum() > 150
        frows, fops, fnorm, _ = _lift(engine, b, w, policy | FUSED)
        _same_norm(fnorm, norm, f"spans at {t_st}")
        compare_hits(frows, fops, *want, f"spans at {t_st} policy {policy} (fused)")
    for max_size in (100, 2**27):
        want = mu.break_paf_regular(b, max_size)
        for policy in (0, ONE_WALK, FUSED, FUSED | ONE_WALK):
            rows, ops, norm, cnt = _brk(engine, b, max_size, policy)
            compare_hits(rows, ops, *want, f"spans at {t_st} break {max_size} policy {policy}")
            if not policy & FUSED:
                assert cnt["n_generic"] == 0


def test_a_record_of_2_pow_32_units_is_refused(engine):
    """one unit more than a regular record may hold: PANIC_OVERFLOW and no rows, next to a record that is clipped as ever"""
    big = mu.spans_record(2**32)
    b = mu.batch_of([(mu.TILE_SMALL, 1000, 5, "+"), (big, 1000, 5, "-"), (mu.TILE_SMALL, 1010, 5, "-")])
    w = (np.zeros(3, np.uint32), np.array([1000, 1005, 2**31], np.uint64), np.array([1003, 1100, 2**31 + 10], np.uint64))
    keep = mu.batch_of([(mu.TILE_SMALL, 1000, 5, "+"), (mu.TILE_SMALL, 1010, 5, "-")])
    want_rows, want_ops = mu.liftover_regular(keep, w)
    want_rows["rec"] *= 2  # (records 0 and 2 of the batch)
    for policy in (0, FUSED):
        rows, ops, norm, cnt = _lift(engine, b, w, policy)
        assert norm["status"].tolist() == [0, mu.PANIC_OVERFLOW, 0], policy
        mine = rows["rec"] == 1
        assert not (rows["status"][mine] == 0).any() and (policy & FUSED or not mine.any()), "rows of the record of 2^32 units"
        compare_hits(rows[~mine], ops, want_rows, want_ops, f"beside the record of 2^32 units, policy {policy}")
        rows, ops, norm, cnt = _brk(engine, b, 100, policy)
        assert norm["status"].tolist() == [0, mu.PANIC_OVERFLOW, 0] and not (rows["status"][rows["rec"] == 1] == 0).any()


def test_the_fused_scan_lane_guard(engine, oracle):
    """64-op records with 2^25 - 1, 2^25 and 2^25 + 1 units in the eight ops of ONE lane (the fused scan hands a record back when a lane
    reaches 2^25: its 64-lane scans could leave 32 bits), and the same eight ops across two lanes, where neither lane reaches it: the
    fused scan's rows are the stand-alone scan's and the reference's on either side of the guard"""
    b, w = lane_case()
    for policy in (MODERN, LEGACY):
        want = mu.liftover_regular(b, w, policy)
        rows, ops, norm, cnt = _lift(engine, b, w, policy)
        assert (norm["flags"] & 1).all() and (cnt["n_generic"] == 0 or policy == LEGACY)
        compare_hits(rows, ops, *want, f"lane records policy {policy}")
        frows, fops, fnorm, fcnt = _lift(engine, b, w, policy | FUSED)
        _same_norm(fnorm, norm, "lane records")
        compare_hits(frows, fops, *want, f"lane records policy {policy} (fused)")
        if policy == MODERN:
            # the route: a record the fused scan hands back is clipped by the generic kernel (HIT_GENERIC on its rows), one it keeps by the
            # stream kernel -- records 1 and 2 hold 2^25 and 2^25 + 1 units in one lane; record 0 holds 2^25 - 1, records 3 .. 5 hold the
            # same eight ops in two lanes
            gen = (frows["flags"] & rustybam_amd.HIT_GENERIC) != 0
            assert not gen[np.isin(frows["rec"], (0, 3, 4, 5))].any(), "a record below the lane guard left the stream kernel"
            assert gen[frows["rec"] == 1].any() and gen[frows["rec"] == 2].any(), "a record at the lane guard stayed on the stream kernel"
            assert fcnt["n_generic"] == gen.sum()
    for max_size in (0, 100):
        want = mu.break_paf_regular(b, max_size)
        for policy in (0, FUSED, FUSED | ONE_WALK):
            rows, ops, _, _ = _brk(engine, b, max_size, policy)
            compare_hits(rows, ops, *want, f"lane records break {max_size} policy {policy}")
    # the record AT the guard once more against the per-base oracle (2^25 units: about 0.6 GB there)
    one = {k: (v[1:2] if k not in ("ops", "op_off") else v) for k, v in b.items()}
    one["ops"], one["op_off"] = b["ops"][64:128], np.array([0, 64], np.uint64)
    _check_liftover(engine, oracle, one, w, MODERN, "the record at the lane guard")


@pytest.mark.parametrize("name", list(TILE_CASES))
def test_the_tile_kernel_guards(engine, name):
    """sR and sQ at 2^31 - 1 | 2^31 and a tile's sum of sR + sQ at 2^32 - 1 | 2^32 (k_tile.hip), the windows on the LAST record of the tile,
    where the tile's running reference total is largest.  Below a guard the tile kernel keeps the tile (phase[3] > 0, phase[4] == 0); at
    it, and for the records of a dozen ops (whose lanes reach 2^25), the results alone are asserted."""
    b, wl, kept = tile_case(name)
    for i, w in enumerate(wl):
        for policy in (FUSED, 0, FUSED | LEGACY):
            rows, ops, norm, cnt = _lift(engine, b, w, policy)
            assert (norm["status"] == 0).all()
            compare_hits(rows, ops, *mu.liftover_regular(b, w, policy & 1), f"{name}, windows {i}, policy {policy}")
            if kept or not policy & FUSED:  # (a tile the fused scan's lane guard hands back goes to the generic kernel)
                assert cnt["n_generic"] == 0 or policy & LEGACY
            if kept:
                assert int(cnt["phase"][3]) > 0 and int(cnt["phase"][4]) == 0, (name, i, policy, cnt["phase"])
    for max_size in (100, 2**27):
        want = mu.break_paf_regular(b, max_size)
        for policy in (FUSED, FUSED | ONE_WALK, 0):
            rows, ops, norm, cnt = _brk(engine, b, max_size, policy)
            compare_hits(rows, ops, *want, f"{name}, break {max_size}, policy {policy}")
            if kept and max_size == 2**27:  # (--max-size 100 cuts a record of several hundred long ops into more pieces than a tile has lanes: handed back)
                assert int(cnt["phase"][3]) > 0 and int(cnt["phase"][4]) == 0, (name, max_size, policy, cnt["phase"])


# ================================================================== 3. the pair row kernel's score guard
BIG = 2**20
GUARD_SCORES = [(BIG, 1, 1), (1, BIG, 3), (3, 1, BIG), (-BIG, 1, 1)]


@pytest.mark.parametrize("policy", [MODERN, LEGACY])
@pytest.mark.parametrize("total", [511, 512, 513])
def test_the_pair_row_kernel_score_guard(engine, oracle, total, policy):
    """pairs whose query spans sum to 511 | 512 | 513 under a score of 2^20: smax * (Lq + Rq) = 2^29 - 2^20 | 2^29 | 2^29 + 2^20.  Below
    the guard the row kernel cuts the pair with its 32-bit sums, at and above it the wave-per-pair kernel does, in 64 bits"""
    b, left, right = mu.guard_pairs(total)
    ob = oracle.Batch(*batch_args(b))
    for scores in GUARD_SCORES:
        rows, out = engine.overlap_split(*batch_args(b), left, right, scores, policy)
        orows, oout = oracle.overlap_split(ob, left, right, scores, policy)
        assert (orows["status"] == 0).all()
        _compare(rows, out, orows, oout, f"guard pairs {total} {scores} policy {policy}")
        assert (rows["_pad"] == 1).all() and (rows["_row"] == (1 if total < 512 else 0)).all(), (total, scores, rows["_pad"], rows["_row"])
    rows, out = engine.overlap_split(*batch_args(b), left, right, (1, 1, 1), policy)  # (small scores: the row kernel's, whatever the spans)
    assert (rows["_row"] == 1).all()


@pytest.mark.parametrize("policy", [MODERN, LEGACY])
def test_the_wave_kernel_sums_in_64_bits(engine, oracle, policy):
    """an overlap of 1500 bases at a score of 2^20: sums of about 1.6e9, inside the reference's i32 and far outside the row kernel's guard"""
    b, left, right = mu.wide_pair()
    ob = oracle.Batch(*batch_args(b))
    top = 0
    for scores in GUARD_SCORES:
        rows, out = engine.overlap_split(*batch_args(b), left, right, scores, policy)
        orows, oout = oracle.overlap_split(ob, left, right, scores, policy)
        assert (orows["status"] == 0).all()
        _compare(rows, out, orows, oout, f"wide pair {scores} policy {policy}")
        assert (rows["_pad"] == 1).all() and (rows["_row"] == 0).all()
        top = max(top, abs(int(orows["split_score"][0])))
    assert top > 2**29  # (a score no 32-bit sum of the row kernel is trusted with)
