"""rb_dev_nucfreq (k_nucfreq.hip) around its tiles, against the oracle, bit-exact: the list walkers past their first tile, the prefix
maximum across its top level, regions that select nothing, coordinates where 32 bits run out, the depth cap's bookkeeping at its limits,
and the resident entry's own contract (workspace size and alignment, nothing written behind an output, results independent of what the
outputs and the workspace held).

Inputs and the resident-buffer harness are in tests/nf_edge_util.py; tests/test_nucfreq_edge_inputs.py proves on the CPU what each input
holds.  One device region is one fetch of the reference (at most 10000 positions), the oracle answers once per distinct region."""
import numpy as np
import pytest

import nf_edge_util as nu
import rustybam_amd
from nf_edge_util import Resident
from nf_util import Reads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


def host_form(engine, rd, regions):
    rg = np.array(regions, np.int64).reshape(-1, 3)
    return engine.nucfreq(*rd.args(), rg[:, 0], rg[:, 1], rg[:, 2])


def list_lengths(res, ws):
    """how many tiles rb_k_nf_tile_desc put on the middle build's list and on the 16-bit build's: the two counts in wide_list, the last
    array of the workspace ([0] and [max_tiles + 1] of max_tiles + 2 words, rounded up to 256 bytes)"""
    max_tiles = res.n_pos // nu.TILE + res.n_rg
    w = ws[res.ws_bytes - (4 * (max_tiles + 2) + 255) // 256 * 256:res.ws_bytes].view(np.uint32)
    return int(w[0]), int(w[max_tiles + 1])


def test_list_walkers_past_their_first_tile(ctx, oracle):
    """more tiles of 128 .. 255 reads than 3 x CUs and more tiles of over 255 reads than 2 x CUs in one call: the workgroups of both list
    walkers come back for further tiles (the cursor, the two-slot hand-over, the counters zeroed again), the lists meet in wide_list"""
    cus = ctx[0].cuda.get_device_properties(0).multi_processor_count
    rd, regions = nu.walker_reads(), nu.walker_regions(max(1100, 3 * cus + 100))
    kinds = nu.tile_kinds(nu.plan_tiles(rd, regions))
    res = Resident(ctx, rd, regions)
    counts, status, ctr = res.run(0xEE)
    n_wide, n_16 = list_lengths(res, res.last["ws"])
    assert (n_wide, n_16) == (int((kinds == 2).sum()), int((kinds == 0).sum()))
    assert n_wide > 3 * cus and n_16 > 2 * cus, "a list no longer than its grid: no workgroup takes a second tile"
    cov, cnt = nu.expected(oracle, rd, regions, {})
    nu.compare(counts, regions, cov, cnt, "list walkers")
    assert ctr["n_covered"] == int(cov.sum()) and ctr["cap_overflow"] == 0 and ctr["n_dropped"] == 0 and ctr["unsorted"] == 0
    assert ctr["max_depth"] > 255 and (status == rustybam_amd.RD_OK).all()
    counts2, status2, ctr2 = res.run(0x11)
    assert counts2.tobytes() == counts.tobytes() and status2.tobytes() == status.tobytes() and ctr2 == ctr
    assert res.inputs_unchanged()


@pytest.mark.parametrize("name", list(nu.TOP_CASES))
def test_prefix_maximum_across_the_top_level(engine, oracle, name):
    """64 blocks of 2048 reads (one turn of rb_k_nf_pmax_top), 65 (the carry into the second turn), 72 with a second long read in block 70
    and 88 with it in block 50 (where a lost carry misleads the search for a tile's first read): a long read at index 5 reaches every tile
    down the file, and must not reach contig 1"""
    rd, regions, f = nu.top_input(name)
    counts, status, ctr = host_form(engine, rd, regions)
    cov, cnt = nu.expected(oracle, rd, regions)
    nu.compare(counts, regions, cov, cnt, name)
    assert ctr["n_covered"] == int(cov.sum()) and ctr["cap_overflow"] == 0 and ctr["n_dropped"] == 0 and ctr["n_bad"] == 0
    assert (status == rustybam_amd.RD_OK).all() and ctr["max_depth"] == 5      # (contig 1's five reads; on contig 0 a tiny read under the long ones)
    for i, r, e in f["tails"]:      # the long read's last seven bases came out
        o = sum(en - st for _t, st, en in regions[:r])
        assert (counts[o + 5:o + 12] & 0x7FFFFFFF).sum(axis=1).tolist() == [1] * 7


def test_nothing_selected(ctx, oracle):
    """runs of empty regions at the front, in the middle and at the end, tids without reads, tid -1, regions beyond a contig's last read, one-
    position regions, more than 256 regions; counts prefilled with 0xEE: every word of every region is written, zero where nothing is"""
    rd, regions, f = nu.nothing_input()
    res = Resident(ctx, rd, regions)
    counts, status, ctr = res.run(0xEE)
    cov, cnt = nu.expected(oracle, rd, regions, {})
    nu.compare(counts, regions, cov, cnt, "nothing selected")
    assert not (counts == 0xEEEEEEEE).any()
    assert ctr["n_covered"] == int(cov.sum()) and ctr["n_bad"] == 0 and ctr["unsorted"] == 0 and ctr["cap_overflow"] == 0
    assert status.tolist() == [rustybam_amd.RD_OK] * (rd.n - f["n_unplaced"]) + [rustybam_amd.RD_FILTERED] * f["n_unplaced"]
    assert res.inputs_unchanged()


def test_high_coordinates(engine, ctx, oracle):
    """reads that start just below 2^31 and end past it, one read that reaches 2^32 - 2 (its contribution worked out by hand), two reads
    the device declines (a span of 2^31, pos = 2^31): RB_RD_BAD_CIGAR, counted in n_bad, nothing of them in the counts"""
    rd, regions, f = nu.high_input()
    cov, cnt = nu.high_expected(oracle)
    want = np.zeros(rd.n, np.uint32)
    want[f["declined"]] = rustybam_amd.RD_BAD_CIGAR
    for what, (counts, status, ctr) in (("host form", host_form(engine, rd, regions)), ("resident form", Resident(ctx, rd, regions).run(0xEE))):
        nu.compare(counts, regions, cov, cnt, f"high coordinates, {what}")
        assert np.array_equal(status, want) and ctr["n_bad"] == 2 and ctr["unsorted"] == 0 and ctr["cap_overflow"] == 0
        assert ctr["n_covered"] == int(cov.sum())


def test_depth_cap_15360_buffered(engine, oracle):
    """8000 reads on position 0 and one more per start position up to 7360: 15360 buffered, the most rb_k_nf_admit holds -- still the oracle's"""
    rd = nu.cap_input()
    counts, status, ctr = host_form(engine, rd, [nu.CAP_REGION])
    cov, cnt = nu.expected(oracle, rd, [nu.CAP_REGION])
    nu.compare(counts, [nu.CAP_REGION], cov, cnt, "15360 buffered")
    assert ctr["cap_overflow"] == 0 and ctr["max_depth"] == nu.LIVE_MAX and ctr["n_dropped"] == 736 and ctr["n_covered"] == int(cov.sum())


def test_depth_cap_15361_is_reported(engine, ctx):
    """one more start position: cap_overflow from the resident form, RB_E_INVALID from the host form; nothing behind the sentinels (run() checks)"""
    rd = nu.cap_input(n_starts=7361)
    counts, status, ctr = Resident(ctx, rd, [nu.CAP_REGION]).run(0xEE)
    assert ctr["cap_overflow"] == 1 and (status == rustybam_amd.RD_OK).all()
    with pytest.raises(rustybam_amd.RbError):
        host_form(engine, rd, [nu.CAP_REGION])


def test_depth_cap_filtered_reads_in_the_fetch(engine, oracle):
    """300 duplicate-flagged reads among the first 8000 of position 0: they never enter the buffer, the cap is reached 300 records later"""
    rd = nu.cap_input(n_filtered=300)
    counts, status, ctr = host_form(engine, rd, [nu.CAP_REGION])
    cov, cnt = nu.expected(oracle, rd, [nu.CAP_REGION])
    nu.compare(counts, [nu.CAP_REGION], cov, cnt, "filtered reads in a deep fetch")
    assert ctr["cap_overflow"] == 0 and ctr["max_depth"] == nu.LIVE_MAX and ctr["n_dropped"] == 736
    assert np.array_equal(status == rustybam_amd.RD_FILTERED, rd.flag == 0x400)


@pytest.mark.parametrize("n_regions", [64, 200])
def test_depth_cap_drop_pool(ctx, oracle, n_regions):
    """identical deep regions: 64 fit the pool of dropped-read bitmaps (the header's promise); 200 either fit or are reported, never wrong in silence"""
    rd, regions = nu.pool_reads(), [(0, 0, 100)] * n_regions
    counts, status, ctr = Resident(ctx, rd, regions).run(0xEE)
    if n_regions <= 64:
        assert ctr["cap_overflow"] == 0
    if ctr["cap_overflow"] == 0:
        cov, cnt = nu.expected(oracle, rd, regions, {})
        nu.compare(counts, regions, cov, cnt, f"{n_regions} deep regions")
        assert ctr["n_dropped"] == 100 * n_regions and ctr["max_depth"] == nu.DEPTH_CAP and ctr["n_covered"] == int(cov.sum())
    else:
        assert ctr["cap_overflow"] == 1


def test_resident_entry_contract(ctx, oracle):
    """ws_bytes one short and a workspace off by 128 bytes are refused with nothing written; with exactly ws_bytes the results are the
    oracle's, nothing is written behind counts, read_status, counters or the workspace, the inputs stay as they were, and neither what the
    outputs nor what the workspace held before shows in any output byte"""
    rd, regions = nu.contract_input()
    res = Resident(ctx, rd, regions)
    assert res.ws_bytes % 256 == 0
    for bad in (dict(ws_short=1), dict(ws_shift=128)):
        with pytest.raises(rustybam_amd.RbError):
            res.run(0xEE, **bad)
        assert res.outputs_untouched() and res.inputs_unchanged(), bad
    counts, status, ctr = res.run(0xEE)
    cov, cnt = nu.expected(oracle, rd, regions, {})
    nu.compare(counts, regions, cov, cnt, "resident entry")
    assert ctr["n_covered"] == int(cov.sum()) and ctr["unsorted"] == 0 and ctr["cap_overflow"] == 0 and ctr["n_dropped"] == 0
    assert np.array_equal(status == rustybam_amd.RD_FILTERED, (rd.flag & 0x704) != 0) and set(status.tolist()) <= {rustybam_amd.RD_OK, rustybam_amd.RD_FILTERED}
    assert res.inputs_unchanged()
    counts2, status2, ctr2 = res.run(0x11)
    assert counts2.tobytes() == counts.tobytes() and status2.tobytes() == status.tobytes() and ctr2 == ctr
    assert res.inputs_unchanged()


def test_resident_entry_without_regions_or_reads(ctx):
    rd, regions = nu.contract_input()
    for fill in (0xEE, 0x11):
        res = Resident(ctx, rd, [])                       # no regions: the reads' statuses and counters still come out
        counts, status, ctr = res.run(fill)
        assert counts.shape == (0, 4) and np.array_equal(status == rustybam_amd.RD_FILTERED, (rd.flag & 0x704) != 0)
        assert ctr == dict(max_depth=0, n_covered=0, n_bad=0, unsorted=0, n_dropped=0, cap_overflow=0)
        res = Resident(ctx, Reads([], [], [], [], []), regions)    # no reads: every word of every region zero
        counts, status, ctr = res.run(fill)
        assert counts.shape == (res.n_pos, 4) and not counts.any() and len(status) == 0
        assert ctr == dict(max_depth=0, n_covered=0, n_bad=0, unsorted=0, n_dropped=0, cap_overflow=0)
        res = Resident(ctx, Reads([], [], [], [], []), [])
        counts, status, ctr = res.run(fill)
        assert counts.shape == (0, 4) and ctr == dict(max_depth=0, n_covered=0, n_bad=0, unsorted=0, n_dropped=0, cap_overflow=0)
