"""The tile kernel (rustybam_amd/csrc/k_tile.hip) on inputs placed on its constants: the cuts of its set-up (hits that fill the lanes, the
longest run of records it can take), the seams of its stream (head, steps, edge and plain form, ring slots, record starts at every place of
a lane's eight ops) and the gaps of a batch in RB_LIFT_OP_STARTS form.  tests/tile_seam_util.py builds the inputs and restates the set-up's
decisions, tests/test_tile_seam_inputs.py proves on the CPU what the inputs hold.  Every comparison is against the per-base oracle,
integer-exact, rows and clipped CIGARs, with tiles and without; every test asserts its route: counters.phase[3] is the number of tiles
rb_plan_tiles_host cuts, phase[4] -- the records the tile kernel handed to the per-record kernel -- is the model's count, n_generic is 0.
Most of the kernel's guards end in a hand-back, after which the rows are right anyway: only the exact count notices a guard that is off by one.

Families: A stream geometry, B hits fill the lanes and slot classes, C the run cut, D gaps of chosen lengths (device batches, built by hand:
tile_seam_util.starts_batch), E break-paf's long indels on either side of record seams and gaps.

Mutations this file was run against, each a library variant (loaded through RB_VARIANT, built with the commands of tools/mkvariant.sh from an
edited copy of k_tile.hip kept outside the tree), the whole file (131 tests) once per variant; only decisions and sums were changed, never an address, a bound or a mask:
  1. `inc0 <= RBT_HITS` -> `<` (and `> RBT_HITS` -> `>=` on the tile's sum) in setup(): 6 fail, all of family B -- a tile of exactly 64 hits,
     the 64th hit as the last hit of record 15, a first record of 64 hits, each under both scan policies.  Route only: the rows stay right.
  2. `> RBT_GAP_MAX` -> `>=`: 11 fail -- family D's gap of 1024 ops (liftover, break-paf in one walk and in two) and family E's starts-form
     tile, which holds such a gap (8).  Route only.
  3. verdict, `(uint32_t)q < bqj` -> `<=`: 113 fail -- A 21, B 20, C 18, D 30, E 24: every tile of two records and more goes back as a whole.
  4. verdict, the `gmj` term dropped: 38 fail -- D 30 and E's starts-form tile (8): a gap op in front of a record start in its chunk is counted.
  5. run search, `prev = bb + 1u` -> `prev = bb`: 14 fail, all of family C under policy 0 (liftover 7, break-paf 7): every case whose kept
     run does not start the tile.
  6. edge step, `(uint32_t)(idx0 + q) < n_tile` -> `<=`: 120 fail -- A 21, B 22, C 20, D 33, E 24: the op behind the tile's last one is summed.
  With the product library all 131 pass.  Every variant passed tools/check_ring.py's check of its assembly before it ran.
"""
import numpy as np
import pytest

import rustybam_amd
import tile_seam_util as u
from devutil import DevBatch
from rbtest_util import batch_args, compare_hits
from test_gpu_parity import _rebuild_from_descriptor
from test_gpu_tile import tile_env

pytestmark = pytest.mark.gpu

MODERN, LEGACY, FUSED, ONE = rustybam_amd.BSEARCH_MODERN, rustybam_amd.BSEARCH_LEGACY, rustybam_amd.LIFT_FUSED_SCAN, rustybam_amd.BREAK_ONE_WALK
STARTS, DESC = rustybam_amd.LIFT_OP_STARTS, rustybam_amd.LIFT_DESCRIPTORS


@pytest.fixture(scope="module")
def ctx():
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    yield torch, eng, dev
    eng.close()


def route(cnt, n_tiles, back, what, generic=0):
    got = (int(cnt["phase"][3]), int(cnt["phase"][4]), int(cnt["n_generic"]))
    print(f"{what}: tiles {got[0]} (plan {n_tiles}), handed back {got[1]} (model {back}), generic {got[2]}")
    assert got[0] == n_tiles, f"{what}: {got[0]} tiles, the plan has {n_tiles}"
    assert got[1] == back, f"{what}: {got[1]} records handed back, the model says {back}"
    if generic is not None:
        assert got[2] == generic, f"{what}: {got[2]} hits went to the generic kernel"


def descriptors_to_ops(b, rows, ops):
    """rows of RB_LIFT_DESCRIPTORS -> (rows, ops) with every described clip rebuilt from the record's CIGAR"""
    rows, out, at = rows.copy(), [], 0
    for i, g in enumerate(rows):
        if int(g["status"]) != 0:
            continue
        off = int(g["out_off"])
        c = _rebuild_from_descriptor(b, g, ops[off:off + 4]) if int(g["flags"]) & rustybam_amd.HIT_DESCRIPTOR else ops[off:off + int(g["out_n"])]
        assert len(c) == int(g["out_n"])
        rows["out_off"][i] = at
        out.append(c)
        at += len(c)
    return rows, np.concatenate(out) if out else np.zeros(0, np.uint32)


class Host:
    """a dense batch through the host entry points: tiles == no tiles == the oracle"""

    def __init__(self, engine, oracle, b):
        self.engine, self.oracle, self.b = engine, oracle, b
        self.ob = oracle.Batch(*batch_args(b), b["contig"])
        self.status = oracle.normalize(self.ob)["status"]
        self.n_tiles = len(u.plan_tiles(b["op_off"]))

    def _both(self, call, want, what):
        orows, oops = want
        res = []
        for on in (True, False):
            with tile_env(on):
                rows, ops, norm, cnt = call()
            assert np.array_equal(norm["status"], self.status), f"{what}: norm.status"
            keep = (self.status == 0)[rows["rec"]] if len(rows) else np.zeros(0, bool)
            assert (rows["status"][~keep] != 0).all(), what
            res.append((rows[keep], ops, cnt))
        assert int(res[1][2]["phase"][3]) == 0, f"{what}: tiles were made with RB_TILE=0"
        return res

    def liftover(self, w, policy, what, back=None, generic=0):
        want = self.oracle.liftover(self.ob, *w, policy=policy & 1)
        res = self._both(lambda: self.engine.liftover(*batch_args(self.b), self.b["contig"], *w, policy=policy), want, what)
        for (rows, ops, cnt), how in zip(res, ("tiles", "per record")):
            if policy & DESC:
                rows, ops = descriptors_to_ops(self.b, rows, ops)
            compare_hits(rows, ops, *want, f"{what} ({how})")
        if back is not None:
            route(res[0][2], self.n_tiles, back, what, generic)
        return want[0]

    def break_paf(self, max_size, policy, what, back=None, generic=0):
        want = self.oracle.break_paf(self.ob, max_size, policy=policy & 1)
        res = self._both(lambda: self.engine.break_paf(*batch_args(self.b), max_size, policy=policy), want, what)
        for (rows, ops, cnt), how in zip(res, ("tiles", "per record")):
            compare_hits(rows, ops, *want, f"{what} ({how})")
            assert cnt["redo_two_walk"] == 0
        if back is not None:
            route(res[0][2], self.n_tiles, back, what, generic)


class Dev:
    """a device-resident batch (DevBatch.run: sentinels behind rows_cap, out_cap and the workspace): a dense one, or one in starts form
    with its dense twin, whose norm rows it takes"""

    def __init__(self, ctx, oracle, b, starts=None):
        torch, eng, dev = ctx
        self.oracle, self.torch = oracle, torch
        self.twin_b = b if starts is None else starts["twin"]
        self.ob = oracle.Batch(*batch_args(self.twin_b), self.twin_b["contig"])
        self.status = oracle.normalize(self.ob)["status"]
        self.twin = DevBatch(torch, eng, dev, self.twin_b)
        self.dev, self.extra = self.twin, 0
        self.n_tiles = len(u.plan_tiles(b["op_off"] if starts is None else starts["b"]["op_off"]))
        if starts is not None:
            torch.cuda.synchronize()
            eng.dev_scan_records(self.twin.view, 0, self.twin.d_norm.data_ptr())
            self.twin.norm_ready = True
            self.dev = DevBatch(torch, eng, dev, starts["b"])          # the ops with the garbage between the records; op_off_host: the OLD offsets
            self.dev.d_off.copy_(torch.from_numpy(starts["starts"].view(np.int64)).to(dev))   # on the device: the table of starts
            self.dev.d_norm.copy_(self.twin.d_norm)                    # first_op counts from op_off[r]: the twin's rows hold as they are
            self.dev.norm_ready = True
            self.extra = STARTS
            torch.cuda.synchronize()

    def _check(self, d, rows, out, cnt, want, what):
        assert cnt["redo_two_walk"] == 0 and cnt["overflow"] == 0, what
        r, o = d.host_rows(rows, out)
        keep = (self.status == 0)[r["rec"]] if len(r) else np.zeros(0, bool)
        assert (r["status"][~keep] != 0).all(), what
        compare_hits(r[keep], o, *want, what)

    def run(self, what, windows=None, max_size=None, policy=MODERN, back=None, generic=0):
        """the batch under policy (| RB_LIFT_OP_STARTS when it has that form) and its dense twin under policy, both against the oracle"""
        want = self.oracle.liftover(self.ob, *windows, policy=policy & 1) if max_size is None else self.oracle.break_paf(self.ob, max_size, policy=policy & 1)
        cap = len(want[0]) + 4 * len(self.status) + 64
        rows, out, cnt = self.dev.run(windows, policy=policy | self.extra, max_size=max_size, rows_cap=cap)
        self._check(self.dev, rows, out, cnt, want, what)
        if self.dev is not self.twin:
            self._check(self.twin, *self.twin.run(windows, policy=policy, max_size=max_size, rows_cap=cap), want, what + " (the dense twin)")
        if back is not None:
            route(cnt, self.n_tiles, back, what, generic)


# ---- A. stream geometry


@pytest.fixture(scope="module")
def fam_a(engine, oracle):
    out = []
    for k in range(len(u.A_HEADS)):
        b, where, _ = u.family_a(k)
        out.append((Host(engine, oracle, b), u.windows_in_turn(b, where)))
    return out


@pytest.mark.parametrize("policy", [0, FUSED])
@pytest.mark.parametrize("k", range(len(u.A_HEADS)))
def test_heads_and_steps_liftover(fam_a, k, policy):
    h, w = fam_a[k]
    h.liftover(w, policy, f"A head {u.A_HEADS[k]} policy {policy}", back=0)
    h.liftover(w, policy | LEGACY, f"A head {u.A_HEADS[k]} policy {policy}, legacy")


@pytest.mark.parametrize("policy", [0, FUSED])
@pytest.mark.parametrize("k", range(len(u.A_HEADS)))
def test_heads_and_steps_break(fam_a, k, policy):
    h, _ = fam_a[k]
    h.break_paf(u.BREAK_A, policy, f"A head {u.A_HEADS[k]} break policy {policy}", back=0)
    h.break_paf(u.BREAK_A, policy | LEGACY, f"A head {u.A_HEADS[k]} break policy {policy}, legacy")


def test_heads_and_steps_device_batch(ctx, oracle):
    """the batch whose end tile ends on gend & 3 == 2, resident: nothing is written behind what the call was told it has"""
    b, where, _ = u.family_a(2)
    d = Dev(ctx, oracle, b)
    d.run("A device liftover", windows=u.windows_in_turn(b, where), policy=MODERN, back=0)
    d.run("A device break", max_size=u.BREAK_A, policy=MODERN | ONE, back=0)


# ---- B. hits fill the lanes; slot classes


@pytest.fixture(scope="module")
def fam_b(engine, oracle):
    b, where = u.b_batch()
    return Host(engine, oracle, b), where


@pytest.mark.parametrize("policy", [FUSED, 0])
@pytest.mark.parametrize("name", list(u.B_CASES))
def test_hits_fill_the_lanes(fam_b, oracle, name, policy):
    h, where = fam_b
    w = u.b_windows(h.b, where, name)
    back = u.expected_back(oracle, h.b, oracle.liftover(h.ob, *w)[0])
    h.liftover(w, policy, f"B {name} policy {policy}", back=back)
    if policy == 0:
        h.liftover(w, DESC, f"B {name} descriptors", back=back)
    h.liftover(w, policy | LEGACY, f"B {name} policy {policy}, legacy")


# ---- C. the run cut


def irregular(b):
    """the records whose hits are the generic kernel's (n_generic counts them: the only hits of this file that go there)"""
    return np.array([not u.bs.is_regular(c, ends=False) for c in u.records(b)])   # (an end indel is stripped, not walked)


@pytest.mark.parametrize("name", list(u.C_CASES))
def test_run_cut_liftover(engine, oracle, name):
    b, where, w = u.c_case(name)
    h = Host(engine, oracle, b)
    orows = oracle.liftover(h.ob, *w)[0]
    back = u.expected_back(oracle, b, orows)
    h.liftover(w, 0, f"C {name}", back=back, generic=int(u.hits_per_record(orows, len(h.status), h.status)[irregular(b)].sum()))
    h.liftover(w, FUSED, f"C {name}, fused scan")   # (an irregularity in the middle of a record is found behind the stream: results only)
    h.liftover(w, LEGACY, f"C {name}, legacy")


@pytest.mark.parametrize("name", list(u.C_CASES))
def test_run_cut_break(engine, oracle, name):
    b, where, w = u.c_case(name)
    h = Host(engine, oracle, b)
    h.break_paf(50, 0, f"C {name} break", back=u.expected_back(oracle, b, max_size=50), generic=int(irregular(b).sum()))   # (one piece each)
    h.break_paf(50, FUSED, f"C {name} break, fused scan")


# ---- D. RB_LIFT_OP_STARTS: gaps of chosen lengths


@pytest.fixture(scope="module")
def fam_d(ctx, oracle):
    out = {}
    for name in u.D_CASES:
        s = u.d_case(name)
        out[name] = (Dev(ctx, oracle, None, starts=s), s)
    return out


@pytest.mark.parametrize("name", list(u.D_CASES))
def test_gaps_liftover(fam_d, oracle, name):
    d, s = fam_d[name]
    w = u.windows_in_turn(s["twin"], [(s["first"], s["cnt"])])
    back = u.expected_back(oracle, s["twin"], oracle.liftover(d.ob, *w)[0], gaps=s["gaps"], op_off=s["b"]["op_off"])
    assert back == u.D_BACK.get(name, 0)
    d.run(f"D {name}", windows=w, policy=MODERN, back=back)
    d.run(f"D {name}, legacy", windows=w, policy=LEGACY)


@pytest.mark.parametrize("walk", [ONE, 0])
@pytest.mark.parametrize("name", list(u.D_CASES))
def test_gaps_break(fam_d, oracle, name, walk):
    d, s = fam_d[name]
    back = u.expected_back(oracle, s["twin"], max_size=u.BREAK_A, gaps=s["gaps"], op_off=s["b"]["op_off"], two_walk=not walk)
    assert back == u.D_BACK.get(name, 0)
    d.run(f"D {name} break walk {walk}", max_size=u.BREAK_A, policy=MODERN | walk, back=back)


# ---- E. break form across seams and gaps


@pytest.fixture(scope="module")
def fam_e(ctx, oracle):
    return Dev(ctx, oracle, u.e_dense()[0]), Dev(ctx, oracle, None, starts=u.e_starts())


@pytest.mark.parametrize("policy", [ONE, FUSED | ONE, 0, FUSED])
@pytest.mark.parametrize("max_size", u.E_SIZES)
def test_long_indels_beside_record_seams(fam_e, max_size, policy):
    fam_e[0].run(f"E dense max_size {max_size} policy {policy}", max_size=max_size, policy=policy, back=0)


@pytest.mark.parametrize("walk", [ONE, 0])
@pytest.mark.parametrize("max_size", u.E_SIZES)
def test_long_indels_beside_gaps(fam_e, max_size, walk):
    fam_e[1].run(f"E starts max_size {max_size} walk {walk}", max_size=max_size, policy=MODERN | walk, back=0)
