"""rb_dev_swap with out_ops == batch->ops (rb_k_swap_inplace) against oracle.swap: the WHOLE array is compared, guard words in front of and
behind the batch included, so a store one word outside a record shows.  The out-of-place kernel is never the reference; its result is
compared as well, to show that it did not change.  What the inputs hold is proven in tests/test_qbed_inputs.py."""
import numpy as np
import pytest

import qbed_util as qu

pytestmark = pytest.mark.gpu

BATCHES = {b[0]: b[1:] for b in qu.swap_batches()}


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's answer for every batch, computed once"""
    return {k: qu.oracle_swap_whole(oracle, *b) for k, b in BATCHES.items()}


class Dev:
    """a batch in device memory: the whole array with its guards, op_off, strand"""

    def __init__(self, eng, arr, off, strand):
        import torch
        self.torch, self.eng = torch, eng
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        self.arr, self.off, self.strand = up(np.concatenate([arr, np.zeros(4, np.uint32)])), up(off), up(np.concatenate([strand, np.zeros(8, np.uint8)]))
        self.n, self.n_rec, self.n_ops = len(arr), len(strand), int(off[-1])
        torch.cuda.synchronize()

    def view(self):
        return self.eng.batch_view(self.n_rec, self.n_ops, self.arr.data_ptr(), self.off.data_ptr(), 0, 0, 0, 0, self.strand.data_ptr(), 0)

    def swap(self, out_ptr=None):
        rc = self.eng.dev_swap(self.view(), self.arr.data_ptr() if out_ptr is None else out_ptr)
        self.eng.sync()
        return rc

    def words(self):
        return self.arr.cpu().numpy().view(np.uint32)[:self.n].copy()


def first_difference(got, want, off):
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return None
    r = int(np.searchsorted(off, bad[0], side="right")) - 1
    return dict(word=int(bad[0]), n_bad=len(bad), record=r, at=int(bad[0]) - int(off[max(r, 0)]) if 0 <= r < len(off) - 1 else "guard")


@pytest.mark.parametrize("which", list(BATCHES))
def test_in_place_equals_the_oracle_on_the_whole_array(engine, want, which):
    arr, off, strand = BATCHES[which]
    d = Dev(engine, arr, off, strand)
    assert d.swap() == 0
    assert first_difference(d.words(), want[which], off) is None


@pytest.mark.parametrize("which", ["-", "+"])
def test_in_place_record_by_record(engine, oracle, which):
    """every record of one strand alone in a batch of its own in turn would be many launches: instead the records of one strand, in the
    order of tests/qbed_util.py, each checked by name"""
    recs = [r for r in qu.swap_records() if r[2] == ord(which)]
    arr, off, strand = qu.pack_batch(recs, range(len(recs)), guard_front=8, guard_back=8)
    d = Dev(engine, arr, off, strand)
    assert d.swap() == 0
    got, ref = d.words(), qu.oracle_swap_whole(oracle, arr, off, strand)
    wrong = [recs[i][0] for i in range(len(recs)) if not np.array_equal(got[int(off[i]):int(off[i + 1])], ref[int(off[i]):int(off[i + 1])])]
    assert wrong == [] and np.array_equal(got, ref)


def test_swap_twice_restores_the_batch(engine, want):
    arr, off, strand = BATCHES["all"]
    d = Dev(engine, arr, off, strand)
    assert d.swap() == 0
    assert np.array_equal(d.words(), want["all"]) and not np.array_equal(d.words(), arr)
    assert d.swap() == 0
    assert first_difference(d.words(), arr, off) is None  # '+' and '-' records alike: the swap is an involution


def test_out_of_place_is_unchanged(engine, want):
    arr, off, strand = BATCHES["all"]
    g = int(off[0])
    got = engine.swap(arr[g:int(off[-1])], off - np.uint64(g), strand)
    assert np.array_equal(got, want["all"][g:int(off[-1])])
    assert np.array_equal(engine.swap(arr[g:int(off[-1])], off - np.uint64(g), strand, in_place=True), got)  # Engine.swap(in_place=True)
    # on device buffers: the batch itself is left as it was
    import torch
    d = Dev(engine, arr, off, strand)
    out = torch.zeros(len(arr) + 4, dtype=torch.int32, device=d.arr.device)
    torch.cuda.synchronize()
    assert d.swap(out.data_ptr()) == 0
    assert np.array_equal(d.words(), arr)
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[g:int(off[-1])], want["all"][g:int(off[-1])])


@pytest.mark.parametrize("shift", [4, 4 * 1000, -4])
def test_overlapping_output_is_refused(engine, shift):
    arr, off, strand = BATCHES["all"]
    d = Dev(engine, arr, off, strand)
    base = d.arr.data_ptr()
    if shift < 0:  # an output that begins in front of the ops and reaches into them: the view's ops begin one word into the array
        v = d.view()
        v.ops = base + 4
        rc = engine.dev_swap(v, base)
    else:
        rc = d.swap(base + shift)
    engine.sync()
    assert rc == qu.E_INVALID
    assert b"overlap" in engine.L.rb_ctx_last_error(engine.ctx)
    assert np.array_equal(d.words(), arr)  # no kernel ran
