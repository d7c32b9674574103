"""rb_dev_stats_rows (k_hitstats.hip) against the oracle: the reduce row of every hit row's clip, where the clip lies.

The reference is pyoracle.reduce of the clips expanded to plain ops (tests/hitstats_util.py), compared field by field, the three f32
ratios bitwise.  tests/test_hitstats_inputs.py proves on the CPU what the inputs hold.  Memory: out_ops ends with the last clip rounded up
to four words, the batch's ops with the next multiple of 32; a sentinel lies behind the stats rows and behind both arrays."""
import numpy as np
import pytest

import hitstats_util as hu
import rustybam_amd
from devutil import DevBatch
from rbtest_util import compare_hits, digest_rows

pytestmark = pytest.mark.gpu
DESC = rustybam_amd.HIT_DESCRIPTOR
SENT_ROWS = 3


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


def stats_of(ctx, view, rows_ptr, n_rows, out_ptr):
    """one rb_dev_stats_rows call into a buffer with SENT_ROWS rows of 0xEE behind stats[n_rows]: -> the rows; the sentinel must be untouched"""
    torch, eng, dev = ctx
    d_stats = torch.full(((n_rows + SENT_ROWS) * 72,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.dev_stats_rows(view, rows_ptr, n_rows, out_ptr, d_stats.data_ptr())
    torch.cuda.synchronize()
    h = d_stats.cpu().numpy()
    assert (h[n_rows * 72:] == 0xEE).all(), "a stats row was written at or behind stats[n_rows]"
    return h[:n_rows * 72].view(rustybam_amd.REDUCE_DT).copy()


class HandMade:
    """the hand-made rows resident in HBM: out_ops and the batch's ops in buffers that end where the contract says, a sentinel behind each"""

    def __init__(self, ctx):
        torch, eng, dev = ctx
        H = self.H = hu.hand_made()
        self.n_out, self.n_ops = len(H.out_ops), (len(H.ops) + 31) // 32 * 32
        out = np.concatenate([H.out_ops, np.full(1024, 0xEEEEEEEE, np.uint32)])
        ops = np.concatenate([H.ops, np.full(self.n_ops - len(H.ops) + 1024, 0xEEEEEEEE, np.uint32)])
        self.host = (out, ops)
        self.d_out = torch.from_numpy(out.view(np.int32)).to(dev)
        self.d_ops = torch.from_numpy(ops.view(np.int32)).to(dev)
        self.d_off = torch.from_numpy(H.op_off.view(np.int64)).to(dev)
        self.d_rows = torch.from_numpy(H.rows.view(np.uint8)).to(dev)
        self.view = eng.batch_view(len(H.op_off) - 1, len(H.ops), self.d_ops.data_ptr(), self.d_off.data_ptr(), 0, 0, 0, 0, 0, 0)

    def unchanged(self):
        return (np.array_equal(self.d_out.cpu().numpy().view(np.uint32), self.host[0]) and np.array_equal(self.d_ops.cpu().numpy().view(np.uint32), self.host[1])
                and np.array_equal(self.d_rows.cpu().numpy(), self.H.rows.view(np.uint8)))


@pytest.fixture(scope="module")
def hand(ctx):
    return HandMade(ctx)


def test_hand_made_rows(ctx, oracle, hand):
    """every length at every word offset, both forms of the kernel side by side in a wavefront, descriptors of every kind, all nine op codes,
    continuation words, wrong spans, rows that are not OK"""
    H = hand.H
    want = hu.oracle_stats(oracle, H.rows, H.clips)
    got = stats_of(ctx, hand.view, hand.d_rows.data_ptr(), len(H.rows), hand.d_out.data_ptr())
    for k in np.nonzero([any(got[f][i] != want[f][i] for f in hu.STAT_FIELDS + ("flags",)) for i in range(len(got))])[0][:8]:
        print(f"row {k} ({H.kind[k]}, {0 if H.clips[k] is None else len(H.clips[k])} ops at {H.rows['out_off'][k]}): device {got[k]} oracle {want[k]}")
    hu.compare_stats(got, want, "hand-made rows")
    assert hand.unchanged(), "the call wrote to its inputs"
    again = stats_of(ctx, hand.view, hand.d_rows.data_ptr(), len(H.rows), hand.d_out.data_ptr())
    assert again.tobytes() == got.tobytes(), "two calls on the same rows wrote different bytes"


def test_every_prefix_of_a_wavefront(ctx, oracle, hand):
    """n_rows that fill a wavefront's four rows and a block's sixteen only in part, and n_rows = 0"""
    torch, eng, dev = ctx
    H = hand.H
    want = hu.oracle_stats(oracle, H.rows, H.clips)
    for n in (1, 2, 3, 5, 15, 17, 33):
        hu.compare_stats(stats_of(ctx, hand.view, hand.d_rows.data_ptr(), n, hand.d_out.data_ptr()), want[:n], f"the first {n} rows")
    assert len(stats_of(ctx, hand.view, hand.d_rows.data_ptr(), 0, hand.d_out.data_ptr())) == 0
    eng.dev_stats_rows(hand.view, 0, 0, 0, 0)  # n_rows == 0 needs no arrays
    torch.cuda.synchronize()


def test_host_array_form(ctx, oracle, hand):
    """Engine.stats_rows: the same rows through uploads of its own"""
    torch, eng, dev = ctx
    H = hand.H
    hu.compare_stats(eng.stats_rows(H.ops, H.op_off, H.rows, H.out_ops), hu.oracle_stats(oracle, H.rows, H.clips), "Engine.stats_rows")
    assert len(eng.stats_rows(H.ops, H.op_off, H.rows[:0], H.out_ops)) == 0


_dev_batch = {}


def real_batch(ctx, oracle):
    if "D" not in _dev_batch:
        torch, eng, dev = ctx
        _dev_batch["D"] = DevBatch(torch, eng, dev, hu.real_input(oracle).b)
    return _dev_batch["D"]


def check_real(ctx, D, rows, out, t, descriptors, what):
    """the rows equal the oracle's (as the parity tests check), then their stats equal the oracle's reduce of the oracle's clips"""
    r, o = D.host_rows(rows, out)
    if descriptors:  # (clips are stored as descriptors: the digest expands them)
        assert len(r) == len(t.rows) and D.digest(rows, out) == digest_rows(t.rows, t.ops), f"{what}: rows or clips differ from the oracle's"
        ok = r["status"] == 0
        assert (r["flags"][ok] & DESC).any() and not (r["flags"][ok] & DESC).all(), f"{what}: descriptor rows and rows with real ops are both wanted"
    else:
        compare_hits(r, o, t.rows, t.ops, what)
        assert not (r["flags"] & DESC).any()
    got = stats_of(ctx, D.view, rows.data_ptr(), len(r), out.data_ptr())
    hu.compare_stats(got, t.stats, what)
    again = stats_of(ctx, D.view, rows.data_ptr(), len(r), out.data_ptr())
    assert again.tobytes() == got.tobytes(), f"{what}: two calls on the same rows wrote different bytes"


@pytest.mark.parametrize("legacy", [False, True], ids=["modern", "legacy"])
@pytest.mark.parametrize("descriptors", [False, True], ids=["ops", "descriptors"])
def test_rows_of_liftover(ctx, oracle, descriptors, legacy):
    inp, D = hu.real_input(oracle), real_batch(ctx, oracle)
    policy = (rustybam_amd.BSEARCH_LEGACY if legacy else rustybam_amd.BSEARCH_MODERN) | rustybam_amd.LIFT_FUSED_SCAN
    policy |= rustybam_amd.LIFT_DESCRIPTORS if descriptors else 0
    rows, out, cnt = D.run(inp.windows, policy)
    assert int(cnt["n_generic"]) > 0
    check_real(ctx, D, rows, out, hu.real_truth(oracle, legacy), descriptors, f"liftover ({'descriptors' if descriptors else 'ops'}, {'legacy' if legacy else 'modern'})")


@pytest.mark.parametrize("max_size", [0, 100])
@pytest.mark.parametrize("descriptors", [False, True], ids=["ops", "descriptors"])
def test_rows_of_break_paf(ctx, oracle, descriptors, max_size):
    D = real_batch(ctx, oracle)
    policy = rustybam_amd.BSEARCH_MODERN | rustybam_amd.LIFT_FUSED_SCAN | (rustybam_amd.LIFT_DESCRIPTORS if descriptors else 0)
    rows, out, cnt = D.run(None, policy, max_size=max_size, rows_cap=20_000)
    check_real(ctx, D, rows, out, hu.real_truth(oracle, False, max_size), descriptors, f"break-paf --max-size {max_size} ({'descriptors' if descriptors else 'ops'})")
