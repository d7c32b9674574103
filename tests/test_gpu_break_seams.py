"""break-paf's cut detection (liftover.rs:182-226) on inputs placed on the geometry of its three kernels: rb_k_break_pieces (k_misc.hip: the
two-walk path and the list mode for declined records), the BRK build of rb_stream_record (rb_stream.h: the one-walk path for long records)
and the BRK build of the tile kernel (k_tile.hip).  tests/break_seam_util.py builds the inputs, tests/test_break_seam_inputs.py proves on
the CPU what they hold.  Every comparison is against the per-base oracle, integer-exact, rows and clipped CIGARs, and every test asserts
its route.

The policies 0 / LIFT_FUSED_SCAN / BREAK_ONE_WALK / both are given to rb_dev_break on a device-resident batch (tests/devutil.py): the host
wrapper rb_host_break (Engine.break_paf) adds BREAK_ONE_WALK to every policy, so through it the two-walk path never runs.  Family E also
goes through Engine.break_paf, with tiles and without (test_gpu_tile.break_both).

Mutations this file was run against, each a library variant (tools/mkvariant.sh, RB_VARIANT) in which the strict `>` of the long-indel
test is `>=`, so that the device behaves exactly as at --max-size - 1; the whole file (120 tests) once per variant:
  * `> p.max_size` -> `>=` in rb_k_break_pieces (k_misc.hip): 20 fail, the rest pass -- family A at --max-size BIG under the two-walk
    policies (6), B at BIG two-walk (2), C two-walk (2), E on the device batch two-walk (6) and F at BIG under all four policies (4: the
    pieces of a declined record are rb_k_break_pieces' in list mode).  No test of a one-walk policy on regular records fails: there the
    kernel does not run.
  * `> brk_max_` -> `>=` in rb_stream.h, BRK build of k_liftover_brk.hip: 16 fail -- A at BIG under the one-walk policies (6), B at BIG
    one-walk (2), C one-walk (2) and E through Engine.break_paf (6: its run without tiles is the stream kernel's).
  * `> brk_max_` -> `>=` in k_tile.hip: 12 fail, all of family E -- through Engine.break_paf (6) and on the device batch under the one-walk
    policies (6).
"""
import numpy as np
import pytest

import break_seam_util as u
import rustybam_amd
from devutil import DevBatch
from rbtest_util import batch_args, compare_hits
from test_gpu_tile import break_both, tile_env

pytestmark = pytest.mark.gpu

MODERN, LEGACY, FUSED, ONE = rustybam_amd.BSEARCH_MODERN, rustybam_amd.BSEARCH_LEGACY, rustybam_amd.LIFT_FUSED_SCAN, rustybam_amd.BREAK_ONE_WALK
POLICIES = [0, FUSED, ONE, FUSED | ONE]
TWO_WALK = [0, FUSED]


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


class Data:
    """a family's batch on the host and on the device, and the oracle's rows per (max_size, search policy), computed once and left unchanged"""

    def __init__(self, ctx, oracle, b):
        self.oracle, self.b = oracle, b
        self.ob = oracle.Batch(*batch_args(b), b["contig"])
        self.dev = DevBatch(*ctx, b)
        self.status = oracle.normalize(self.ob)["status"]
        self._rows = {}

    def want(self, max_size, legacy=0):
        if (max_size, legacy) not in self._rows:
            self._rows[max_size, legacy] = self.oracle.break_paf(self.ob, max_size, policy=legacy)
        return self._rows[max_size, legacy]

    def run(self, max_size, policy, what, ordered=False):
        """rb_dev_break under `policy` against the oracle, on the records the oracle keeps; -> (rows, counters)"""
        orows, oops = self.want(max_size, policy & 1)
        rows, out, cnt = self.dev.run(max_size=max_size, policy=policy, rows_cap=len(orows) + 4 * len(self.status) + 64)
        assert cnt["redo_two_walk"] == 0 and cnt["overflow"] == 0, what
        r, o = self.dev.host_rows(rows, out)
        self.dev.torch.cuda.synchronize()
        norm = self.dev.d_norm.cpu().numpy().view(rustybam_amd.NORM_DT)["status"][:len(self.status)]
        assert np.array_equal(norm, self.status), f"{what}: norm.status"
        keep = (self.status == 0)[r["rec"]] if len(r) else np.zeros(0, bool)
        assert (r["status"][~keep] != 0).all(), f"{what}: rows of records the reference panics on must carry a status"
        r = r[keep]
        compare_hits(r, o, orows, oops, what)
        if ordered:  # rows of one record in piece order, win counting up from 0
            rec, win = r["rec"].astype(np.int64), r["win"].astype(np.int64)
            first = np.concatenate([[True], rec[1:] != rec[:-1]])
            assert (np.diff(rec) >= 0).all() and (win[first] == 0).all() and (win[1:][~first[1:]] == win[:-1][~first[1:]] + 1).all(), what
        return r, cnt


@pytest.fixture(scope="module")
def fam_a(ctx, oracle):
    return {v: (Data(ctx, oracle, u.family_a(v)[0]), u.family_a(v)[1]) for v in u.VARIANTS}


@pytest.fixture(scope="module")
def fam_b(ctx, oracle):
    fam = u.family_b()
    return Data(ctx, oracle, u.make_batch([c for c, _, _ in fam.values()])), [p for _, p, _ in fam.values()]


# ---- A. seams of the layouts


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("max_size", u.MAX_SIZES)
@pytest.mark.parametrize("variant", u.VARIANTS)
def test_long_indels_at_the_seams(fam_a, variant, max_size, policy):
    d, idx = fam_a[variant]
    rows, cnt = d.run(max_size, policy, f"seams {variant} max_size={max_size} policy={policy}", ordered=True)
    per = np.bincount(rows["rec"].astype(np.int64), minlength=len(d.status))[idx]
    assert cnt["n_generic"] == 0
    if max_size == u.BIG:
        assert (per == 1).all()   # the comparison is strict
    elif max_size == 0:
        assert per.min() > 20 * u.PASS
    else:
        assert per.min() >= 9


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("variant", u.VARIANTS)
def test_long_indels_at_the_seams_legacy(fam_a, variant, policy):
    d, idx = fam_a[variant]
    d.run(100, policy | LEGACY, f"seams {variant} legacy policy={policy}", ordered=True)


# ---- B. pass boundaries of the stream kernel


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("max_size", [100, u.BIG - 1, u.BIG])
def test_cuts_at_the_pass_boundaries(fam_b, max_size, policy):
    d, pieces = fam_b
    rows, cnt = d.run(max_size, policy, f"passes max_size={max_size} policy={policy}", ordered=True)
    per = np.bincount(rows["rec"].astype(np.int64), minlength=len(pieces)).tolist()
    assert per == (pieces if max_size < u.BIG else [1] * len(pieces))
    assert cnt["n_generic"] == 0 and int(cnt["phase"][3]) == 0


@pytest.mark.parametrize("policy", POLICIES)
def test_one_op_piece_at_a_pass_boundary(ctx, oracle, policy):
    """the records of test_gpu_break_onewalk.py::test_many_pieces_in_several_passes, against the oracle, on the per-record kernel"""
    for tiny_at in (31, 63, 33):
        d = Data(ctx, oracle, u.make_batch([u.tiny_record(tiny_at)], strands="+" if tiny_at != 63 else "-"))
        with tile_env(False):
            rows, cnt = d.run(100, policy, f"tiny_at={tiny_at} policy={policy}", ordered=True)
        assert len(rows) == 71 and cnt["n_generic"] == 0 and int(cnt["phase"][3]) == 0


# ---- C. record ends


@pytest.mark.parametrize("policy", POLICIES)
def test_long_indel_runs_around_the_body(ctx, oracle, policy):
    b, ends = u.family_c()
    d = Data(ctx, oracle, b)
    assert (d.status == 0).sum() >= 8
    for max_size in (100, u.BIG, 0):
        rows, cnt = d.run(max_size, policy, f"record ends max_size={max_size} policy={policy}")
        assert len(rows) >= (d.status == 0).sum()


# ---- D. the collect cap of rb_k_break_pieces


@pytest.mark.parametrize("policy", TWO_WALK)
@pytest.mark.parametrize("n_cut", u.CAP_CUTS)
def test_single_record_at_the_collect_cap(ctx, oracle, n_cut, policy):
    d = Data(ctx, oracle, u.make_batch([u.cap_record(n_cut)]))
    with tile_env(False):
        rows, cnt = d.run(100, policy, f"cap {n_cut} cuts policy={policy}", ordered=True)
    assert len(rows) == n_cut + 1 and cnt["n_generic"] == 0 and int(cnt["phase"][3]) == 0


@pytest.mark.parametrize("tiles", [False, True])
@pytest.mark.parametrize("policy", TWO_WALK)
def test_cap_records_among_neighbours(ctx, oracle, policy, tiles):
    b, want = u.family_d_batch()
    d = Data(ctx, oracle, b)
    with tile_env(tiles):
        rows, cnt = d.run(100, policy, f"cap batch policy={policy} tiles={tiles}", ordered=True)
    assert np.bincount(rows["rec"].astype(np.int64)).tolist() == want and cnt["n_generic"] == 0
    assert (int(cnt["phase"][3]) > 0) == tiles


# ---- E. tiles


@pytest.mark.parametrize("policy", [ONE, FUSED | ONE])
@pytest.mark.parametrize("pieces", [u.TILE_HITS - 1, u.TILE_HITS, u.TILE_HITS + 1])
def test_tile_with_63_64_65_pieces(engine, oracle, pieces, policy):
    b = u.family_e(pieces)
    cnt = break_both(engine, oracle, b, 100, policy, f"tile of {pieces} pieces policy={policy}")
    assert int(cnt["phase"][3]) > 0 and (int(cnt["phase"][4]) > 0) == (pieces > u.TILE_HITS), (pieces, cnt["phase"])
    assert cnt["n_generic"] == 0 and cnt["redo_two_walk"] == 0
    cnt = break_both(engine, oracle, b, u.BIG, policy, f"tile of {pieces} pieces, nothing cut, policy={policy}", expect_back=0)
    assert cnt["n_generic"] == 0


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("pieces", [u.TILE_HITS - 1, u.TILE_HITS, u.TILE_HITS + 1])
def test_tile_with_63_64_65_pieces_device_batch(ctx, oracle, pieces, policy):
    d = Data(ctx, oracle, u.family_e(pieces))
    for max_size in (100, u.BIG):
        with tile_env(True):
            rows, cnt = d.run(max_size, policy, f"tile of {pieces} pieces max_size={max_size} policy={policy}", ordered=True)
        assert len(rows) == (pieces if max_size == 100 else len(d.status)) and cnt["n_generic"] == 0 and int(cnt["phase"][3]) > 0
        assert (int(cnt["phase"][4]) > 0) == (pieces > u.TILE_HITS and max_size == 100), (pieces, max_size, cnt["phase"])


# ---- F. declined records


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("max_size", [100, u.BIG, 0])
def test_soft_clipped_records_are_declined_one_by_one(ctx, oracle, max_size, policy):
    b, idx = u.family_a("behind", soft=True)
    d = Data(ctx, oracle, b)
    assert (d.status == 0).all()
    rows, cnt = d.run(max_size, policy, f"declined max_size={max_size} policy={policy}", ordered=True)
    per = np.bincount(rows["rec"].astype(np.int64), minlength=len(d.status))[idx]
    assert cnt["n_generic"] >= per.sum() > 0
    assert (per == 1).all() if max_size == u.BIG else per.min() >= 9
