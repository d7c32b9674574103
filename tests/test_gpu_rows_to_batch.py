"""rb_dev_rows_to_batch (k_rows_batch.hip) against its numpy model (tests/rows_batch_util.py), bit for bit: the hit rows of a clip call as a
dense batch of records.  tests/test_rows_batch_inputs.py proves on the CPU what the inputs hold and that the model is the contract.

Memory: every output lies in a buffer that goes on behind the capacity the call is told, filled with a sentinel; out_ops ends with the last
clip rounded up to four words, the batch's ops with the next multiple of 32."""
from types import SimpleNamespace

import numpy as np
import pytest

import rows_batch_util as ru
import rustybam_amd
from devutil import DevBatch

pytestmark = pytest.mark.gpu
DESC = rustybam_amd.HIT_DESCRIPTOR
SENT = 0xEE
TAIL = 64  # elements of sentinel behind every capacity


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


def call(ctx, view, rows_ptr, n_rows, out_ptr, pieces_cap, ops_cap, sizes_only=False):
    """ONE rb_dev_rows_to_batch call that is told pieces_cap and ops_cap, on buffers TAIL elements longer and full of 0xEE: -> the buffers as
    the call left them (host copies, whole), info, and `tails_ok`: nothing at or behind a capacity, the info block or the scratch was written"""
    torch, eng, dev = ctx
    sizes = dict(ops=(ops_cap, 4), op_off=(pieces_cap + 1, 8), t_st=(pieces_cap, 8), t_en=(pieces_cap, 8), q_st=(pieces_cap, 8), q_en=(pieces_cap, 8),
                 strand=(pieces_cap, 1), contig=(pieces_cap, 4), parent=(pieces_cap, 4))
    d = {k: torch.full(((n + TAIL) * w,), SENT, dtype=torch.uint8, device=dev) for k, (n, w) in sizes.items()}
    scr_bytes = eng.rows_to_batch_scratch_bytes(n_rows)
    d_scr = torch.full((scr_bytes + 4096,), SENT, dtype=torch.uint8, device=dev)
    d_info = torch.full((64 + 256,), SENT, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.dev_rows_to_batch(view, rows_ptr, n_rows, out_ptr, pieces_cap, ops_cap, 0 if sizes_only else d["ops"].data_ptr(), d["op_off"].data_ptr(),
                          [d[k].data_ptr() for k in ("t_st", "t_en", "q_st", "q_en")], d["strand"].data_ptr(), d["contig"].data_ptr(),
                          d["parent"].data_ptr(), d_info.data_ptr(), d_scr.data_ptr())
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    info = d_info.cpu().numpy()
    tails = {k: bool((h[k][sizes[k][0] * sizes[k][1]:] == SENT).all()) for k in h}
    tails["info"] = bool((info[64:] == SENT).all())
    tails["scratch"] = bool((d_scr[scr_bytes:] == SENT).all().item())
    dt = dict(ops=np.uint32, op_off=np.uint64, t_st=np.uint64, t_en=np.uint64, q_st=np.uint64, q_en=np.uint64, strand=np.uint8, contig=np.uint32, parent=np.uint32)
    return SimpleNamespace(raw=h, dev=d, info=info[:64].view(rustybam_amd.PIECES_INFO_DT)[0].copy(), tails=tails, tails_ok=all(tails.values()),
                           arr={k: h[k][:sizes[k][0] * sizes[k][1]].view(dt[k]) for k in h})


def check(r, m, what):
    """a call that fitted: counts, every array bit for bit, nothing else written"""
    assert r.tails_ok, f"{what}: written behind a capacity: {[k for k, v in r.tails.items() if not v]}"
    assert (int(r.info["n_pieces"]), int(r.info["n_ops"])) == (m.n_pieces, m.n_ops), f"{what}: info {r.info}"
    assert r.info["overflow"] == 0 and (r.info["_reserved"] == 0).all(), f"{what}: info {r.info}"
    got = r.arr["ops"][:m.n_ops]
    bad = np.nonzero(got != m.ops)[0]
    if len(bad):
        p = int(np.searchsorted(m.op_off, bad[0], side="right")) - 1
        print(f"{what}: first wrong word {bad[0]} (piece {p}, word {bad[0] - int(m.op_off[p])} of {int(m.op_off[p + 1] - m.op_off[p])}): {got[bad[0]]:#x} != {m.ops[bad[0]]:#x}; {len(bad)} wrong")
    assert len(bad) == 0, f"{what}: ops differ"
    assert (r.raw["ops"][m.n_ops * 4:] == SENT).all(), f"{what}: a word was written behind new_ops[n_ops]"
    assert np.array_equal(r.arr["op_off"][:m.n_pieces + 1], m.op_off), f"{what}: op_off"
    assert (r.raw["op_off"][(m.n_pieces + 1) * 8:] == SENT).all(), f"{what}: written behind new_op_off[n_pieces]"
    for k in ru.PIECE_FIELDS[1:]:
        assert np.array_equal(r.arr[k][:m.n_pieces], getattr(m, k)), f"{what}: {k}"
        assert (r.raw[k][m.n_pieces * r.arr[k].itemsize:] == SENT).all(), f"{what}: {k} written behind [n_pieces]"


class Resident:
    """rows, out_ops and the batch they point into, resident in HBM in buffers that end where the contract says"""

    def __init__(self, ctx, rows, out_ops, ops, op_off, strand, contig):
        torch, eng, dev = ctx
        self.rows = rows
        out = np.concatenate([out_ops, np.zeros(-len(out_ops) % 4, np.uint32)])
        opsp = np.concatenate([ops, np.zeros(-len(ops) % 32, np.uint32)])
        self.host = (out, opsp)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev)  # noqa: E731
        self.d_out, self.d_ops, self.d_off, self.d_rows = up(out if len(out) else np.zeros(4, np.uint32)), up(opsp), up(op_off), up(rows if len(rows) else np.zeros(1, rustybam_amd.HIT_DT))
        self.d_strand, self.d_contig = up(strand), up(contig)
        self.view = eng.batch_view(len(strand), len(ops), self.d_ops.data_ptr(), self.d_off.data_ptr(), 0, 0, 0, 0, self.d_strand.data_ptr(), self.d_contig.data_ptr())

    def call(self, ctx, n_rows, pieces_cap, ops_cap, **kw):
        return call(ctx, self.view, self.d_rows.data_ptr(), n_rows, self.d_out.data_ptr(), pieces_cap, ops_cap, **kw)

    def unchanged(self):
        return (np.array_equal(self.d_out.cpu().numpy().view(np.uint32)[:len(self.host[0])], self.host[0]) and np.array_equal(self.d_ops.cpu().numpy().view(np.uint32), self.host[1])
                and (len(self.rows) == 0 or np.array_equal(self.d_rows.cpu().numpy(), self.rows.view(np.uint8))))


@pytest.fixture(scope="module")
def hand(ctx):
    H = ru.hand_made()
    return SimpleNamespace(H=H, R=Resident(ctx, H.rows, H.out_ops, H.ops, H.op_off, H.strand, H.contig))


def test_hand_made_rows(ctx, hand):
    """every threshold length at every source and destination word offset, both forms of the kernel side by side in a wavefront, descriptors
    of every kind, continuation words, rows that are not OK; and two calls write the same bytes"""
    H, R = hand.H, hand.R
    m = H.model
    r = R.call(ctx, len(H.rows), m.n_pieces, m.n_ops)
    check(r, m, "hand-made rows")
    assert r.info["declined"] == 0
    assert R.unchanged(), "the call wrote to its inputs"
    again = R.call(ctx, len(H.rows), m.n_pieces, m.n_ops)
    assert all(again.raw[k].tobytes() == r.raw[k].tobytes() for k in r.raw) and again.info.tobytes() == r.info.tobytes(), "two calls wrote different bytes"


def test_every_prefix_of_the_rows(ctx, hand):
    """n_rows = 0 .. 65: a wavefront's four rows and a block's sixteen filled only in part, and no rows at all"""
    torch, eng, dev = ctx
    H, R = hand.H, hand.R
    ok = H.rows["status"] == 0
    for n in range(66):
        m = ru.prefix(H.model, int(ok[:n].sum()))
        check(R.call(ctx, n, m.n_pieces, m.n_ops), m, f"the first {n} rows")
    d_info = torch.full((64,), SENT, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.dev_rows_to_batch(R.view, 0, 0, 0, 0, 0, 0, 0, None, 0, 0, 0, d_info.data_ptr(), 0)  # n_rows == 0, sizes only: needs no arrays
    torch.cuda.synchronize()
    assert (d_info.cpu().numpy() == 0).all()


def test_sizes_only(ctx, hand):
    """new_ops == NULL: info is written and nothing else"""
    H, R = hand.H, hand.R
    r = R.call(ctx, len(H.rows), H.model.n_pieces, H.model.n_ops, sizes_only=True)
    assert (int(r.info["n_pieces"]), int(r.info["n_ops"]), int(r.info["overflow"]), int(r.info["declined"])) == (H.model.n_pieces, H.model.n_ops, 0, 0)
    assert r.tails_ok and all((v == SENT).all() for v in r.raw.values()), "a sizes-only call wrote to an output"
    r = R.call(ctx, len(H.rows), 0, 0, sizes_only=True)  # (the capacities are not looked at)
    assert (int(r.info["n_pieces"]), int(r.info["n_ops"]), int(r.info["overflow"])) == (H.model.n_pieces, H.model.n_ops, 0)


@pytest.mark.parametrize("short", ["pieces", "ops", "both", "one-of-each", "nothing"])
def test_short_capacities(ctx, hand, short):
    """the capacity contract: nothing at or behind pieces_cap, ops_cap or the end of the scratch; RB_OK, overflow and exact counts; the retry
    with exactly those counts fits"""
    H, R = hand.H, hand.R
    m = H.model
    pc, oc = {"pieces": (m.n_pieces - 1, m.n_ops), "ops": (m.n_pieces, m.n_ops - 1), "both": (m.n_pieces // 2, m.n_ops // 3 + 1),
              "one-of-each": (1, 1), "nothing": (0, 0)}[short]
    r = R.call(ctx, len(H.rows), pc, oc)
    assert r.tails_ok, f"written behind a capacity: {[k for k, v in r.tails.items() if not v]}"
    assert (int(r.info["n_pieces"]), int(r.info["n_ops"])) == (m.n_pieces, m.n_ops) and r.info["overflow"] != 0, f"info {r.info}"
    check(R.call(ctx, len(H.rows), int(r.info["n_pieces"]), int(r.info["n_ops"])), m, "the retry with the reported counts")
    assert R.unchanged()


def test_rows_that_decline(ctx, hand):
    """a panic status, or a replaced length that needs a continuation word, sets declined; their neighbours below the line do not; the
    pieces are the model's either way"""
    H = hand.H
    for what, rows, out, m in ru.declining():
        R = Resident(ctx, rows, out, H.ops, H.op_off, H.strand, H.contig)
        r = R.call(ctx, len(rows), m.n_pieces, m.n_ops)
        check(r, m, what)
        assert bool(r.info["declined"]) == m.declined, f"{what}: declined = {r.info['declined']}"
        r = R.call(ctx, len(rows), 0, 0, sizes_only=True)
        assert bool(r.info["declined"]) == m.declined, f"{what} (sizes only): declined = {r.info['declined']}"


_asm = {}


def asm_batch(ctx):
    if "D" not in _asm:
        torch, eng, dev = ctx
        _asm["D"] = DevBatch(torch, eng, dev, ru.asm_small())
    return _asm["D"]


def break_rows(ctx, max_size, descriptors):
    """the rows and clips of rb_dev_break on asm_small.paf, left on the device: -> (rows tensor, out tensor, host rows, host out_ops)"""
    key = (max_size, descriptors)
    if key not in _asm:
        D = asm_batch(ctx)
        policy = rustybam_amd.BSEARCH_MODERN | rustybam_amd.LIFT_FUSED_SCAN | (rustybam_amd.LIFT_DESCRIPTORS if descriptors else 0)
        rows, out, cnt = D.run(None, policy, max_size=max_size, rows_cap=40_000)
        r, o = D.host_rows(rows, out)
        _asm[key] = (rows, out, r.copy(), o.copy())
    return _asm[key]


@pytest.mark.parametrize("max_size", [100, 7])
@pytest.mark.parametrize("descriptors", [False, True], ids=["ops", "descriptors"])
def test_rows_of_break_paf(ctx, oracle, descriptors, max_size):
    """asm_small.paf: the pieces of the device's break-paf rows are the model's, and -- the rows being the oracle's -- the oracle's pieces;
    then the round trip: the piece batch through rb_dev_scan_records says of every piece what rb_dev_stats_rows says of its row, and
    normalises to itself"""
    torch, eng, dev = ctx
    D, b = asm_batch(ctx), ru.asm_small()
    rows, out, r, o = break_rows(ctx, max_size, descriptors)
    if descriptors:
        assert (r["flags"][r["status"] == 0] & DESC).any()
    m = ru.model(r, o, b["ops"], b["op_off"], b["strand"], b["contig"])
    ob = oracle.Batch(b["ops"], b["op_off"], b["t_st"], b["t_en"], b["q_st"], b["q_en"], b["strand"], b["contig"])
    orows, oops = oracle.break_paf(ob, max_size)
    om = ru.model(rustybam_amd.capi.hit_rows_from(orows), oops, b["ops"], b["op_off"], b["strand"], b["contig"])
    assert m.n_pieces == om.n_pieces and np.array_equal(m.ops, om.ops) and np.array_equal(m.op_off, om.op_off) and np.array_equal(m.parent, om.parent)
    res = call(ctx, D.view, rows.data_ptr(), len(r), out.data_ptr(), m.n_pieces, m.n_ops)
    check(res, m, f"break-paf --max-size {max_size}")
    assert res.info["declined"] == 0
    # ---- the round trip ----
    d = res.dev
    view = eng.batch_view(m.n_pieces, m.n_ops, d["ops"].data_ptr(), d["op_off"].data_ptr(), d["t_st"].data_ptr(), d["t_en"].data_ptr(), d["q_st"].data_ptr(),
                          d["q_en"].data_ptr(), d["strand"].data_ptr(), d["contig"].data_ptr())
    d_red = torch.zeros(m.n_pieces * 72, dtype=torch.uint8, device=dev)
    d_norm = torch.zeros(m.n_pieces * 64, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(len(r) * 72, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.dev_scan_records(view, d_red.data_ptr(), d_norm.data_ptr())
    eng.dev_stats_rows(D.view, rows.data_ptr(), len(r), out.data_ptr(), d_stats.data_ptr())
    torch.cuda.synchronize()
    red, norm = d_red.cpu().numpy().view(rustybam_amd.REDUCE_DT), d_norm.cpu().numpy().view(rustybam_amd.NORM_DT)
    stats = d_stats.cpu().numpy().view(rustybam_amd.REDUCE_DT)[r["status"] == 0]
    for f in rustybam_amd.REDUCE_DT.names:
        if f != "flags":
            assert red[f].tobytes() == stats[f].tobytes(), f"reduce rows of the pieces: {f} differs from rb_dev_stats_rows of their rows"
    assert ((red["flags"] & 4) == (stats["flags"] & 4)).all()
    assert (norm["status"] == 0).all() and (norm["first_op"] == 0).all() and np.array_equal(norm["n_ops"], np.diff(m.op_off).astype(np.uint32))
    assert not (norm["flags"] & 2).any(), "a piece came back stripped"
    for f in ("t_st", "t_en", "q_st", "q_en"):
        assert np.array_equal(norm[f], getattr(m, f))


def test_source_batch_in_op_starts_form(ctx):
    """the records' starts shuffled, gaps between them: op_off is a table of starts, extents come from the rows alone"""
    torch, eng, dev = ctx
    b = ru.asm_small()
    rows, out, r, o = break_rows(ctx, 100, True)
    ops2, starts = ru.starts_form(b, np.random.default_rng(11))
    m = ru.model(r, o, b["ops"], b["op_off"], b["strand"], b["contig"])
    m2 = ru.model(r, o, ops2, starts, b["strand"], b["contig"])
    assert np.array_equal(m.ops, m2.ops)
    R = Resident(ctx, r, o, ops2, starts, b["strand"], b["contig"])
    check(call(ctx, R.view, rows.data_ptr(), len(r), out.data_ptr(), m.n_pieces, m.n_ops), m, "RB_LIFT_OP_STARTS form")


def test_host_array_form(ctx, hand):
    """Engine.rows_to_batch: sizes-only call, then the fill with exactly those sizes, through uploads of its own"""
    torch, eng, dev = ctx
    H = hand.H
    got, info = eng.rows_to_batch(H.ops, H.op_off, H.strand, H.contig, H.rows, H.out_ops)
    assert (int(info["n_pieces"]), int(info["n_ops"]), int(info["overflow"])) == (H.model.n_pieces, H.model.n_ops, 0)
    for k in ("ops",) + ru.PIECE_FIELDS:
        assert np.array_equal(got[k], getattr(H.model, k)), k
