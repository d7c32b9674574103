"""trim-paf under the LEGACY binary-search policy on the in-place pair kernels (four pairs per wavefront, the wave-per-pair kernel behind
it): bit-exact against the per-base oracle, on inputs tests/test_trim_legacy_inputs.py shows to tell the policies apart, with the pairs
done where the modern policy's are -- by the fast kernels, in place -- so that the resident pipeline (passes, then break-paf straight off
the batch with RB_LIFT_OP_STARTS) has one shape for both policies."""
import hashlib
import json
import os

import numpy as np
import pytest

import rustybam_amd
from rbtest_util import read_paf
from test_gpu_trim import _compare, _pairs_batch
from trim_legacy_util import INPUTS, LEGACY, MODERN, ROW_FIELDS, SCORES, legacy_batch, odd_geometries, oracle_rows, rows_differ
from trim_util import format_resident

pytestmark = pytest.mark.gpu


def _split(engine, b, left, right, scores, policy):
    return engine.overlap_split(b["ops"], b["op_off"], b["t_st"], b["t_en"], b["q_st"], b["q_en"], b["strand"], left, right, scores, policy)


@pytest.mark.parametrize("scores", SCORES)
@pytest.mark.parametrize("ops_range,n_pairs,max_overlap,floor", INPUTS)
def test_legacy_pairs_equal_the_oracle_and_stay_on_the_fast_kernels(engine, oracle, ops_range, n_pairs, max_overlap, floor, scores):
    """(a) rows and cigars of every pair equal the oracle's under the legacy policy, and at least 3/4 of the pairs carry _pad == 1 (done by
    a wave kernel, not by the serial one).  Before the pair kernels served the policy no legacy pair did."""
    b, left, right = legacy_batch(ops_range, n_pairs, max_overlap, scores)
    rows, out = _split(engine, b, left, right, scores, LEGACY)
    orows, oout = oracle_rows(oracle, b, left, right, scores, LEGACY)
    _compare(rows, out, orows, oout, f"legacy {ops_range} {scores}")
    by_wave = int((rows["_pad"] == 1).sum())
    print(f"legacy {ops_range} {scores}: {by_wave} of {len(rows)} pairs by the wave kernels")
    assert 4 * by_wave >= 3 * len(rows), f"only {by_wave} of {len(rows)} pairs were done by the wave kernels"


def test_legacy_resident_fixture_in_place(golden):
    """(b) asm_small.paf through trim_driver.ResidentTrim under legacy: the oracle CLI's digest, and the share of pairs cut in place that
    test_gpu_trim.py holds the modern policy to."""
    import torch
    from rustybam_amd import trim_driver
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    r = read_paf(os.path.join(golden, "asm_small.paf"))
    rank = {q: i for i, q in enumerate(sorted(set(r.q_name)))}
    group = np.array([rank[q] for q in r.q_name])
    T = trim_driver.ResidentTrim(eng, torch, dev, r.ops, r.op_off, r.t_st, r.t_en, r.q_st, r.q_en, r.strand, group)
    norm0 = T.d_norm.cpu().numpy().view(rustybam_amd.NORM_DT)[:r.n].copy()
    T.run((1, 1, 1), LEGACY)
    print(f"legacy fixture: {T.pairs_by_wave} of {T.pairs_done} pairs by the wave kernels, {T.passes} passes")
    assert T.passes >= 2 and T.pairs_done > 100
    assert T.pairs_by_wave >= 0.95 * T.pairs_done, f"{T.pairs_by_wave} of {T.pairs_done} pairs by the wave kernels"
    d_new, new_off, norm = T.gather()
    lines = format_resident(r, norm0, norm, d_new.cpu().numpy().view(np.uint32), new_off, T.order).splitlines(keepends=True)
    dig = json.load(open(os.path.join(golden, "digests.json")))["trim_paf_legacy"]["md5"]
    assert len(lines) == 249
    assert hashlib.md5("".join(lines).encode()).hexdigest() == dig
    eng.close()


class _SampleCheck:
    """on_pass hook of ResidentTrim.run: a seeded sample of every pass's pairs, spread over the pass, against the per-base oracle.  The
    records of a pass are what the passes before it left: the hook carries every record as a view of the batch's ORIGINAL ops (start,
    count, and the two end words a cut rewrote, read back from the device) and hands the oracle the sampled pairs' records as they were
    BEFORE the pass."""

    def __init__(self, oracle, torch, T, ops_host, h, per_pass, seed):
        self.oracle, self.torch, self.T, self.ops, self.per_pass = oracle, torch, T, ops_host, per_pass
        self.rng = np.random.default_rng(seed)
        self.off = h["op_off"][:-1].astype(np.int64).copy()
        self.n = np.diff(h["op_off"].astype(np.int64))
        self.fw, self.lw = self.ops[self.off].copy(), self.ops[self.off + self.n - 1].copy()
        self.c = {k: h[k].astype(np.uint64).copy() for k in ("t_st", "t_en", "q_st", "q_en")}
        self.strand = h["strand"]
        self.sampled, self.differ, self.per_pass_sampled = 0, 0, []

    def _cigar(self, rec):
        c = self.ops[self.off[rec]:self.off[rec] + self.n[rec]].copy()
        c[0], c[-1] = self.fw[rec], self.lw[rec]  # (first before last, as the kernel writes them: a one-op record holds the last)
        return c

    def __call__(self, i, k, d_l, d_r, d_rows):
        torch = self.torch
        left, right = d_l[:k].cpu().numpy().view(np.uint32).astype(np.int64), d_r[:k].cpu().numpy().view(np.uint32).astype(np.int64)
        rows = d_rows[: k * 128].cpu().numpy().view(rustybam_amd.capi.PAIR_DT)
        assert (rows["status"] == 0).all() and (rows["_pad"] == 1).all(), f"pass {i}: a pair was not cut in place"
        pick = np.sort(self.rng.choice(k, size=min(k, self.per_pass), replace=False))  # uniform over the pass = over the whole batch
        recs = np.stack([left[pick], right[pick]], axis=1).reshape(-1)
        cig = [self._cigar(r) for r in recs]
        off = np.zeros(len(cig) + 1, np.uint64)
        off[1:] = np.cumsum([len(c) for c in cig])
        b = dict(ops=np.concatenate(cig), op_off=off, strand=self.strand[recs], **{f: self.c[f][recs] for f in self.c})
        pl, pr = np.arange(0, 2 * len(pick), 2, dtype=np.uint32), np.arange(1, 2 * len(pick), 2, dtype=np.uint32)
        want, wout = oracle_rows(self.oracle, b, pl, pr, (1, 1, 1), LEGACY)
        modern, _ = oracle_rows(self.oracle, b, pl, pr, (1, 1, 1), MODERN)
        got = rows[pick]
        assert (want["status"] == 0).all()
        for f in ("split_idx", "split_score") + ROW_FIELDS:
            bad = np.nonzero(got[f] != want[f])[0] if got[f].ndim == 1 else np.nonzero((got[f] != want[f]).any(axis=1))[0]
            assert len(bad) == 0, f"pass {i}: {f} of pairs {pick[bad[:5]]} differs from the oracle: device {got[f][bad[:3]]} oracle {want[f][bad[:3]]}"
        # the state after the pass, from the device's rows (every pair of the pass), and the end words its cuts wrote
        d_ops = self.T.d_ops
        for s, rec in ((0, left), (1, right)):
            first = rows["out_off"][:, s].astype(np.int64)
            cnt = rows["out_n"][:, s].astype(np.int64)
            self.off[rec], self.n[rec] = first, cnt
            self.fw[rec] = d_ops[torch.from_numpy(first).to(d_ops.device)].cpu().numpy().view(np.uint32)
            self.lw[rec] = d_ops[torch.from_numpy(first + cnt - 1).to(d_ops.device)].cpu().numpy().view(np.uint32)
            for f in self.c:
                self.c[f][rec] = rows[f][:, s]
        for j, p in enumerate(pick):  # the cigars of the sampled pairs, as they now lie in the batch
            for s, rec in ((0, left[p]), (1, right[p])):
                o, m = int(want["out_off"][j][s]), int(want["out_n"][j][s])
                assert np.array_equal(self._cigar(rec), wout[o:o + m]), f"pass {i}: cigar of pair {p} side {s}"
        self.sampled += len(pick)
        self.per_pass_sampled.append(len(pick))
        self.differ += int(rows_differ(want, modern).sum())


def test_legacy_config4_pipeline_in_place(oracle):
    """(c) the config-4 shape (4 records of 300-700 ops per query, consecutive spans overlapping) under legacy: every pair of every pass cut
    in place, break-paf --max-size 100 straight off the trimmed batch (RB_LIFT_OP_STARTS) equal to break-paf on the gathered dense copy,
    and a seeded sample of 800 pairs of every pass equal to the per-base oracle -- some of them different from their modern rows."""
    import torch
    from rustybam_amd import capi
    from devutil import DevBatch, config4_resident
    n = 200_000
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    eng = rustybam_amd.Engine(0, torch.cuda.current_stream().cuda_stream)
    T, h = config4_resident(torch, eng, dev, n)
    ops_host = capi.synth_fill_ops_host(0x5EED0004, 0, h["op_off"])
    chk = _SampleCheck(oracle, torch, T, ops_host, h, per_pass=800, seed=0x1E6AC4)
    T.run((1, 1, 1), LEGACY, on_pass=chk)
    print(f"legacy config 4: {T.pairs_by_wave} of {T.pairs_done} pairs in place, {T.passes} passes, sampled {chk.per_pass_sampled}, "
          f"{chk.differ} of the sampled pairs differ from their modern rows")
    assert T.pairs_done > n // 2 and T.pairs_by_wave == T.pairs_done
    assert chk.sampled >= 2000 and len(chk.per_pass_sampled) >= 3 and min(chk.per_pass_sampled) >= 600
    assert chk.differ >= 1, "no sampled pair tells the policies apart"
    B = DevBatch.from_trimmed(torch, eng, dev, T)  # (raises if a pass moved a record)
    rows, out, cnt = B.run(None, max_size=100, rows_cap=6 * n, policy=LEGACY | rustybam_amd.LIFT_OP_STARTS | rustybam_amd.BREAK_ONE_WALK)
    assert not cnt["redo_two_walk"] and not cnt["overflow"]
    got, got_digest = B.host_rows(rows, out)[0].copy(), B.digest(rows, out)
    d_new, new_off, norm = T.gather()
    d_c = [torch.from_numpy(np.ascontiguousarray(norm[k]).view(np.int64)).to(dev) for k in ("t_st", "t_en", "q_st", "q_en")]
    G = DevBatch.from_device(torch, eng, dev, d_new, int(new_off[-1]), new_off, d_c, torch.from_numpy(h["strand"]).to(dev))
    rows, out, cnt = G.run(None, max_size=100, rows_cap=6 * n, policy=LEGACY | rustybam_amd.LIFT_FUSED_SCAN | rustybam_amd.BREAK_ONE_WALK)
    assert not cnt["redo_two_walk"] and not cnt["overflow"]
    want, _ = G.host_rows(rows, out)
    assert len(got) == len(want) and len(want) > n // 2
    for k in ("rec", "win", "status", "out_n", "t_st", "t_en", "q_st", "q_en", "nmatch", "aln_len"):
        assert np.array_equal(got[k], want[k]), k
    assert got_digest == G.digest(rows, out)
    del B, G, rows, out
    T.release()
    torch.cuda.synchronize()
    eng.close()


def test_legacy_odd_geometries(engine, oracle):
    """(d) spans that do not overlap, touch, coincide or contain one another under legacy: the pairs go down the chain to the serial kernel
    as before, statuses (the reference's panics) and rows as the oracle's"""
    b, left, right = odd_geometries()
    for scores in ((1, 1, 1), (5, 1, 2)):
        rows, out = _split(engine, b, left, right, scores, LEGACY)
        orows, oout = oracle_rows(oracle, b, left, right, scores, LEGACY)
        assert np.array_equal(rows["status"], orows["status"])
        _compare(rows, out, orows, oout, f"legacy odd geometries {scores}")
    assert len(set(orows["status"].tolist())) >= 2


def test_legacy_unsorted_qpos_array(engine, oracle):
    """(d) q_st == 0 on '+' behind a leading op without query bases: qpos_aln is not sorted and the serial kernel replays the legacy
    search base by base, as before"""
    rng = np.random.default_rng(7002)
    b, left, right = _pairs_batch(rng, 200, "wild", zero_bias=True)
    rows, out = _split(engine, b, left, right, (1, 1, 1), LEGACY)
    orows, oout = oracle_rows(oracle, b, left, right, (1, 1, 1), LEGACY)
    assert (orows["status"] == 16).any() and (orows["status"] == 0).any()
    assert np.array_equal(rows["status"], orows["status"])
    _compare(rows, out, orows, oout, "legacy unsorted qpos")


@pytest.mark.parametrize("ops_range", [(3, 60), (60, 200)])
def test_legacy_runs_of_several_ops(engine, oracle, ops_range):
    """spliced records (D and N side by side: a run of several non-query ops behind a last base, legal in a regular record): the
    four-pairs-per-wavefront kernel hands such a pair on under legacy, the wave-per-pair kernel walks the run -- rows as the oracle's
    under both policies, and the inputs hold such runs and tell the policies apart"""
    rng = np.random.default_rng(4242 + ops_range[0])
    b, left, right = _pairs_batch(rng, 300, "spliced", ops_range=ops_range)
    opc = b["ops"] & 15
    nonq = (opc == 2) | (opc == 3)
    assert int((nonq[1:] & nonq[:-1]).sum()) > 50  # (a few of these pairs of neighbours straddle two records: the count is a floor on nothing but "many")
    res = {}
    for policy in (MODERN, LEGACY):
        rows, out = _split(engine, b, left, right, (2, 3, 5), policy)
        orows, oout = oracle_rows(oracle, b, left, right, (2, 3, 5), policy)
        _compare(rows, out, orows, oout, f"spliced {ops_range} policy {policy}")
        res[policy] = orows
    assert int(rows_differ(res[MODERN], res[LEGACY]).sum()) >= 10
